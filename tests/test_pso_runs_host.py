"""PSO / CPSO with options["runs"], host side (no GPU): the C ABI of csrc/sx_pso_runs.hip -- struct mirror, the host-only LDS
budget -- and the argument checks of optimize.minimize(method="pso" / "cpso", options={"runs": R}), all of which raise a
ValueError that names `runs` before a device is needed."""
import ctypes as C
import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _pso_runs_abi  # noqa: E402

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

    assert C.sizeof(_lib.SxPsoRunsArgs) == lib.sx_struct_size(9)
    assert _lib.SxPsoRunsArgs.R.offset == 12 * 8 and _lib.SxPsoRunsArgs.ftol.offset == C.sizeof(_lib.SxPsoRunsArgs) - 8


@pytest.mark.parametrize("P,n", [(4, 3), (32, 32), (64, 128)])
def test_lds_budget_of_shapes_that_fit(lib, P, n):
    """(64, 128): X, V and pbest are 3 * 64 * 128 * 8 = 196 608 bytes, more than the 163 840 a workgroup may declare; such a
    swarm keeps X and pbest in the LDS and its velocities in the workspace."""
    got = lib.sx_pso_runs_lds_bytes(P, n)
    assert 0 < got <= LDS_LIMIT
    work = lib.sx_pso_runs_workspace_bytes(5, P, n)
    assert work in (0, 5 * P * n * 8)
    assert got + work // 5 >= 3 * P * n * 8  # X, V and pbest at the least, in the LDS or beside it
    assert (work == 0) == (3 * P * n * 8 < LDS_LIMIT - 8 * (10 * P + n + 4))


def test_lds_budget_refuses_what_does_not_fit(lib):
    assert lib.sx_pso_runs_lds_bytes(4096, 128) < 0
    assert lib.sx_pso_runs_lds_bytes(1, 8) < 0 and lib.sx_pso_runs_lds_bytes(8, 0) < 0  # not a swarm / not a row
    assert lib.sx_pso_runs_lds_bytes(4, lib.sx_wide_from() + 1) < 0                     # rows the wide kernels serve
    for P, n in ((4096, 128), (1, 8), (8, 0), (4, lib.sx_wide_from() + 1)):
        assert lib.sx_pso_runs_workspace_bytes(3, P, n) < 0
    assert lib.sx_pso_runs_workspace_bytes(0, 4, 3) < 0


R, P, N = 3, 8, 5
BASE = {"runs": R, "popsize": P, "maxiter": 4, "seed": 0, "rng": "philox", "updating": "deferred"}
METHODS = ("pso", "cpso")


def _call(sa, method, fun=None, x0=None, callback=None, n=N, **changes):
    opts = dict(BASE, **changes)
    return sa.optimize.minimize(fun if fun is not None else sa.factory.sphere, [[-5.12, 5.12]] * n, x0=x0, method=method,
                                options=opts, callback=callback)


BAD = {
    "numpy-legacy rng": lambda sa, m: _call(sa, m, rng="numpy-legacy"),
    "default rng": lambda sa, m: _call(sa, m, rng=None),
    "batched objective": lambda sa, m: _call(sa, m, fun=sa.factory.batched(lambda X: (X * X).sum(dim=1))),
    "plain lambda": lambda sa, m: _call(sa, m, fun=lambda x: float(np.sum(x * x))),
    "workers=2": lambda sa, m: _call(sa, m, workers=2),
    "callback": lambda sa, m: _call(sa, m, callback=lambda X, res: None),
    "return_all": lambda sa, m: _call(sa, m, return_all=True),
    "runs=0": lambda sa, m: _call(sa, m, runs=0),
    "runs=-2": lambda sa, m: _call(sa, m, runs=-2),
    "runs=2.5": lambda sa, m: _call(sa, m, runs=2.5),
    "seed sequence of the wrong length": lambda sa, m: _call(sa, m, seed=[1, 2]),
    "no seed": lambda sa, m: _call(sa, m, seed=None),
    "x0 (R+1, P, n)": lambda sa, m: _call(sa, m, x0=np.zeros((R + 1, P, N))),
    "P x n beyond the LDS": lambda sa, m: _call(sa, m, popsize=4096, n=128),
    "rows beyond the narrow kernels": lambda sa, m: _call(sa, m, n=2049),
    "strict immediate": lambda sa, m: _call(sa, m, updating="immediate", strict_updating=True),
}


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("what", sorted(BAD))
def test_argument_checks_name_runs_and_need_no_device(sa, what, method):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # (a plain callable's host-evaluation note is not what is tested)
        with pytest.raises(ValueError, match="runs"):
            BAD[what](sa, method)


@pytest.mark.parametrize("method", METHODS)
def test_immediate_updating_defers_with_a_warning_unless_told_otherwise(sa, method):
    """updating="immediate" cannot be an ordered sweep of R runs: strict_updating=None says so in a warning, False is
    silent; either way the call then goes on -- here into the next check, which needs no device either."""
    with pytest.warns(RuntimeWarning, match="deferred"):
        with pytest.raises(ValueError, match="runs"):
            _call(sa, method, updating="immediate", return_all=False, seed=[1])
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        with pytest.raises(ValueError, match="runs"):
            _call(sa, method, updating="immediate", strict_updating=False, seed=[1])


@pytest.mark.parametrize("method", METHODS)
def test_reference_checks_still_come_first(sa, method):
    """The reference's own argument checks (cpso/_cpso.py:116-145) are not displaced by the new option."""
    with pytest.raises(ValueError):
        _call(sa, method, inertia=1.5)
    with pytest.raises(KeyError):
        _call(sa, method, constraints="Random")
    with pytest.raises(ValueError):
        _call(sa, method, x0=np.zeros((P + 1, N)))


def test_x0_is_checked_per_run_or_shared(sa):
    with pytest.raises(ValueError):
        _call(sa, "pso", x0=np.zeros((P, N + 1)))
    with pytest.raises(ValueError, match="runs"):
        _call(sa, "cpso", x0=np.zeros((R, P, N + 1)))


@pytest.mark.parametrize("n", [3, 64, 256, 257, 1024, 2048])
def test_lds_budget_at_its_limit(lib, sa, n):
    """The largest swarm sx_pso_runs_lds_bytes accepts for rows of n elements: within 160 KiB, one row more refused, and
    everywhere the bytes of the layouts the kernel's header comment documents --
    X[P][stride] | V[P][n] | pbest[P][n] | pbestfit[P] | gbest[n] | rad[P] | 4 broadcast words while that is within 160 KiB
    (no workspace), the same without V above (workspace: R P n doubles); stride = n + 8 up to 256 elements,
    n + 8 + 2 (n // 64 + 2) above (the broadcast words are the LAST bytes of the run's LDS: a budget short of them is a write
    past it).  Strictly increasing inside each layout.  The front end refuses the first swarm that does not fit, before a
    device is needed."""
    pmax = _pso_runs_abi.largest_popsize(lib, n)
    stride = n + 8 if n <= 256 else n + 8 + 2 * (n // 64 + 2)
    assert _pso_runs_abi.stride_doubles(n) == stride
    top = lib.sx_pso_runs_lds_bytes(pmax, n)
    assert 0 < top <= 163840 == LDS_LIMIT
    assert lib.sx_pso_runs_lds_bytes(pmax + 1, n) < 0 and lib.sx_pso_runs_workspace_bytes(2, pmax + 1, n) < 0
    assert 8 * ((pmax + 1) * (stride + n + 2) + n + 4) > LDS_LIMIT  # pmax + 1 is refused because it does not fit without V either
    P = np.arange(2, pmax + 1, dtype=np.int64)
    got = np.array([lib.sx_pso_runs_lds_bytes(p, n) for p in P], dtype=np.int64)
    work = np.array([lib.sx_pso_runs_workspace_bytes(2, p, n) for p in P], dtype=np.int64)
    whole = 8 * (P * (stride + 2 * n + 2) + n + 4)
    inside = whole <= LDS_LIMIT
    assert inside[0] and not inside[-1] and (np.diff(inside.astype(int)) <= 0).all()  # both layouts occur, in this order
    assert np.array_equal(got, np.where(inside, whole, 8 * (P * (stride + n + 2) + n + 4)))
    assert np.array_equal(work, np.where(inside, 0, 2 * P * n * 8))
    assert (np.diff(got[inside]) > 0).all() and (np.diff(got[~inside]) > 0).all()
    assert np.array_equal(got, [_pso_runs_abi.lds_bytes(p, n) for p in P])
    assert np.array_equal(work, [_pso_runs_abi.workspace_bytes(2, p, n) for p in P])
    for method in METHODS:
        with pytest.raises(ValueError, match="runs.*LDS.*160 KiB"):  # the budget check, not an earlier refusal
            _call(sa, method, runs=2, popsize=pmax + 1, n=n)
