"""VD-CMA with options["runs"], host side (no GPU): the C ABI of csrc/sx_vd_runs.hip -- struct mirror, the host-only LDS and
workspace budgets, the two residency conditions -- and the argument checks of optimize.minimize(method="vdcma",
options={"runs": R}), all of which raise a ValueError that names `runs` before a device is needed."""
import ctypes as C
import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _vd_runs_abi as abi  # noqa: E402

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

    assert C.sizeof(_lib.SxVdRunsArgs) == lib.sx_vd_runs_args_bytes() == 16 * 8 + 2 * 8 + 6 * 4 + 11 * 8
    assert _lib.SxVdRunsArgs.R.offset == 16 * 8 and _lib.SxVdRunsArgs.ftol.offset == C.sizeof(_lib.SxVdRunsArgs) - 8
    assert _lib.SxVdRunsArgs.vvec0.offset == 2 * 8 and _lib.SxVdRunsArgs.wsum.offset == _lib.SxVdRunsArgs.sigma.offset - 8
    assert lib.sx_struct_size(11) == -1  # (the new struct has an entry point of its own)


def largest_dim(lib):
    """The largest n the layout takes at the smallest population."""
    return abi.largest(lambda n: lib.sx_vd_runs_lds_bytes(2, n) > 0, 6, lib.sx_wide_from() + 1)


def test_the_largest_dimension(lib):
    nmax = largest_dim(lib)
    assert 512 < nmax < lib.sx_wide_from()
    assert abi.lds_bytes(2, nmax) <= LDS_LIMIT < abi.lds_bytes(2, nmax + 1)
    assert all(lib.sx_vd_runs_lds_bytes(2, n) < 0 for n in range(nmax + 1, lib.sx_wide_from() + 2))


@pytest.mark.parametrize("n", [6, 64, 65, 128, 129, 256, 257, 512, "nmax"])
def test_lds_budget_is_the_documented_layout(lib, sa, n):
    """For P = 2 ... pmax + 1: the bytes of the layout the kernel's header comment documents, never decreasing; the largest
    accepted P is within 160 KiB and P + 1 is refused because it does not fit.  The front end refuses that popsize before a
    device is needed."""
    n = largest_dim(lib) if n == "nmax" else n
    pmax = abi.largest_popsize(lib, n)
    top = lib.sx_vd_runs_lds_bytes(pmax, n)
    assert 0 < top <= 163840 == LDS_LIMIT
    assert lib.sx_vd_runs_lds_bytes(pmax + 1, n) < 0 and abi.lds_bytes(pmax + 1, n) > LDS_LIMIT
    P = np.arange(2, pmax + 1, dtype=np.int64)
    got = np.array([lib.sx_vd_runs_lds_bytes(int(p), n) for p in P], dtype=np.int64)
    assert np.array_equal(got, [abi.lds_bytes(int(p), n) for p in P])
    assert (np.diff(got) >= 0).all() and (got[2:] > got[:-2]).all()
    with pytest.raises(ValueError, match=r"runs.*popsize %d x %d.*160 KiB" % (pmax + 1, n)):  # the budget check, not an earlier one
        _call(sa, runs=2, popsize=pmax + 1, n=n)


def test_the_residency_conditions(lib):
    """popsize = 10 (the API default) for every ndim from 6 to 512; popsize = 4 + floor(3 ln n) for every ndim from 6 to 256."""
    for n in range(6, 513):
        assert lib.sx_vd_runs_lds_bytes(10, n) == abi.lds_bytes(10, n) <= LDS_LIMIT, n
    for n in range(6, 257):
        P = abi.default_popsize(n)
        assert lib.sx_vd_runs_lds_bytes(P, n) == abi.lds_bytes(P, n) <= LDS_LIMIT, n
    assert lib.sx_vd_runs_lds_bytes(32, 600) > 0  # (the longest case of tests/test_gpu_vd_runs.py)


def test_lds_budget_refuses_what_is_not_a_run(lib):
    assert lib.sx_vd_runs_lds_bytes(8, 0) < 0 and lib.sx_vd_runs_lds_bytes(8, 5) < 0 and lib.sx_vd_runs_lds_bytes(8, -3) < 0
    assert lib.sx_vd_runs_lds_bytes(8, 6) > 0
    assert lib.sx_vd_runs_lds_bytes(2, lib.sx_wide_from() + 1) < 0 and lib.sx_vd_runs_lds_bytes(2, 1 << 30) < 0
    assert lib.sx_vd_runs_lds_bytes(1, 8) < 0 and lib.sx_vd_runs_lds_bytes(0, 8) < 0
    assert lib.sx_vd_runs_lds_bytes(1 << 40, 8) < 0


def test_workspace_is_one_history_per_run(lib):
    assert lib.sx_vd_runs_workspace_bytes(16, 100) == abi.workspace_bytes(16, 100) == 16 * 100 * 8
    assert lib.sx_vd_runs_workspace_bytes(0, 100) < 0 and lib.sx_vd_runs_workspace_bytes(3, 0) < 0


R, P, N = 3, 8, 7
BASE = {"runs": R, "popsize": P, "maxiter": 4, "seed": 0, "rng": "philox"}


def _call(sa, fun=None, x0=None, callback=None, n=N, **changes):
    opts = dict(BASE, **changes)
    return sa.optimize.minimize(fun if fun is not None else sa.factory.sphere, [[-3.0, 3.0]] * n, x0=x0, method="vdcma",
                                options=opts, callback=callback)


BAD = {
    "numpy-legacy rng": lambda sa: _call(sa, rng="numpy-legacy"),
    "default rng": lambda sa: _call(sa, rng=None),
    "batched objective": lambda sa: _call(sa, fun=sa.factory.batched(lambda X: (X * X).sum(dim=1))),
    "plain lambda": lambda sa: _call(sa, fun=lambda x: float(np.sum(x * x))),
    "workers=2": lambda sa: _call(sa, workers=2),
    "callback": lambda sa: _call(sa, callback=lambda X, res: None),
    "return_all": lambda sa: _call(sa, return_all=True),
    "Penalize": lambda sa: _call(sa, constraints="Penalize"),
    "runs=0": lambda sa: _call(sa, runs=0),
    "runs=-2": lambda sa: _call(sa, runs=-2),
    "runs=2.5": lambda sa: _call(sa, runs=2.5),
    "runs=True": lambda sa: _call(sa, runs=True),
    "seed sequence of the wrong length": lambda sa: _call(sa, seed=[1, 2]),
    "no seed": lambda sa: _call(sa, seed=None),
    "x0 (R+1, n)": lambda sa: _call(sa, x0=np.zeros((R + 1, N))),
    "x0 (R, n+1)": lambda sa: _call(sa, x0=np.zeros((R, N + 1))),
    "n = 5": lambda sa: _call(sa, n=5),
    "n = 2": lambda sa: _call(sa, n=2),
    "n beyond the layout": lambda sa: _call(sa, n=1500),
    "popsize beyond the LDS": lambda sa: _call(sa, popsize=100000, n=32),
    "popsize 1": lambda sa: _call(sa, popsize=1),
    "maxiter 0": lambda sa: _call(sa, maxiter=0),
}


@pytest.mark.parametrize("what", sorted(BAD))
def test_argument_checks_name_runs_and_need_no_device(sa, what, monkeypatch):
    from stochopy_amd import _device

    def no_device(*a, **k):
        raise AssertionError("a refusal must not need a device")

    monkeypatch.setattr(_device, "Context", no_device)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # (a plain callable's host-evaluation note is not what is tested)
        with pytest.raises(ValueError, match="runs"):
            BAD[what](sa)


def test_the_limit_and_the_shape_are_named(sa):
    with pytest.raises(ValueError, match=r"runs.*ndim >= 6.*ndim = 5.*learning rates.*method='cmaes'"):
        _call(sa, n=5)
    with pytest.raises(ValueError, match=r"runs.*popsize 100000 x 32.*160 KiB"):
        _call(sa, popsize=100000, n=32)
    with pytest.raises(ValueError, match=r"runs.*popsize 8 x 1500.*160 KiB"):
        _call(sa, n=1500)


def test_reference_checks_still_come_first(sa):
    """The reference's own argument checks (_evolution.check_arguments: vdcma/_vdcma.py:143-161) are not displaced by the
    option: they raise as they do without it, whatever else is wrong with the call."""
    with pytest.raises(ValueError) as e:
        _call(sa, sigma=0.0, rng="numpy-legacy")
    assert "runs" not in str(e.value)
    with pytest.raises(ValueError) as e:
        _call(sa, muperc=0.0, rng="numpy-legacy")
    assert "runs" not in str(e.value)
    with pytest.raises(KeyError):
        _call(sa, constraints="Shrink", rng="numpy-legacy")
    with pytest.raises(ValueError) as e:
        _call(sa, x0=np.zeros(N + 1), rng="numpy-legacy")
    assert "runs" not in str(e.value)


def test_runs_one_or_none_is_the_single_call(sa, monkeypatch):
    """runs = None and runs = 1 never enter the batched front end: they construct the single run as before."""
    from stochopy_amd.optimize import _vdcma

    class Single(Exception):
        pass

    def boom(*a, **k):
        raise AssertionError("the batched front end was entered")

    def single(*a, **k):
        raise Single()

    monkeypatch.setattr(_vdcma, "_minimize_runs", boom)
    monkeypatch.setattr(_vdcma, "_VdDeviceRun", single)
    for runs in (None, 1, np.int64(1)):
        with pytest.raises(Single):
            _call(sa, runs=runs)
