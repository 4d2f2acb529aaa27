"""CMA-ES with options["runs"], host side (no GPU): the C ABI of csrc/sx_cma_runs.hip -- struct mirror, the host-only LDS and
workspace budgets -- and the argument checks of optimize.minimize(method="cmaes", options={"runs": R}), all of which raise a
ValueError that names `runs` before a device is needed."""
import ctypes as C
import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _cma_runs_abi  # noqa: E402

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

    assert C.sizeof(_lib.SxCmaRunsArgs) == lib.sx_struct_size(10)
    assert _lib.SxCmaRunsArgs.R.offset == 13 * 8 and _lib.SxCmaRunsArgs.ftol.offset == C.sizeof(_lib.SxCmaRunsArgs) - 8
    assert lib.sx_struct_size(11) == -1


@pytest.mark.parametrize("n", [1, 16, 17, 32])
def test_lds_budget_is_the_documented_layout(lib, sa, n):
    """For P = 2 ... pmax: the bytes of the layout the kernel's header comment documents, strictly increasing once the
    candidates outgrow the Jacobi storage they share their bytes with (never decreasing before); the largest accepted P is
    within 160 KiB and P + 1 is refused because it does not fit.  The front end refuses that popsize before a device is
    needed."""
    pmax = _cma_runs_abi.largest_popsize(lib, n)
    top = lib.sx_cma_runs_lds_bytes(pmax, n)
    assert 0 < top <= 163840 == LDS_LIMIT
    assert lib.sx_cma_runs_lds_bytes(pmax + 1, n) < 0 and _cma_runs_abi.lds_bytes(pmax + 1, n) > LDS_LIMIT
    P = np.arange(2, pmax + 1, dtype=np.int64)
    got = np.array([lib.sx_cma_runs_lds_bytes(int(p), n) for p in P], dtype=np.int64)
    assert np.array_equal(got, [_cma_runs_abi.lds_bytes(int(p), n) for p in P])
    assert (np.diff(got) > 0).all()
    with pytest.raises(ValueError, match="runs.*LDS.*160 KiB"):  # the budget check, not an earlier refusal
        _call(sa, runs=2, popsize=pmax + 1, n=n)


def test_lds_budget_refuses_what_is_not_a_run(lib):
    assert lib.sx_cma_runs_lds_bytes(8, 33) < 0  # beyond the one-workgroup eigensolver
    assert lib.sx_cma_runs_lds_bytes(8, 0) < 0
    assert lib.sx_cma_runs_lds_bytes(1, 8) < 0
    assert lib.sx_cma_runs_lds_bytes(1 << 40, 8) < 0


def test_workspace_is_one_history_per_run(lib):
    assert lib.sx_cma_runs_workspace_bytes(16, 100) == _cma_runs_abi.workspace_bytes(16, 100) == 16 * 100 * 8
    assert lib.sx_cma_runs_workspace_bytes(0, 100) < 0 and lib.sx_cma_runs_workspace_bytes(3, 0) < 0


R, P, N = 3, 8, 5
BASE = {"runs": R, "popsize": P, "maxiter": 4, "seed": 0, "rng": "philox"}


def _call(sa, fun=None, x0=None, callback=None, n=N, **changes):
    opts = dict(BASE, **changes)
    return sa.optimize.minimize(fun if fun is not None else sa.factory.sphere, [[-3.0, 3.0]] * n, x0=x0, method="cmaes",
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
    "eigh=host": lambda sa: _call(sa, eigh="host"),
    "eigh=callable": lambda sa: _call(sa, eigh=np.linalg.eigh),
    "runs=0": lambda sa: _call(sa, runs=0),
    "runs=-2": lambda sa: _call(sa, runs=-2),
    "runs=2.5": lambda sa: _call(sa, runs=2.5),
    "runs=True": lambda sa: _call(sa, runs=True),
    "seed sequence of the wrong length": lambda sa: _call(sa, seed=[1, 2]),
    "no seed": lambda sa: _call(sa, seed=None),
    "x0 (R+1, n)": lambda sa: _call(sa, x0=np.zeros((R + 1, N))),
    "x0 (R, n+1)": lambda sa: _call(sa, x0=np.zeros((R, N + 1))),
    "n = 33": lambda sa: _call(sa, n=33),
    "popsize beyond the LDS": lambda sa: _call(sa, popsize=4096, n=32),
    "popsize 1": lambda sa: _call(sa, popsize=1),
    "maxiter 0": lambda sa: _call(sa, maxiter=0),
}


@pytest.mark.parametrize("what", sorted(BAD))
def test_argument_checks_name_runs_and_need_no_device(sa, what):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # (a plain callable's host-evaluation note is not what is tested)
        with pytest.raises(ValueError, match="runs"):
            BAD[what](sa)


def test_the_limit_and_the_shape_are_named(sa):
    with pytest.raises(ValueError, match=r"runs.*ndim <= 32.*ndim = 40"):
        _call(sa, n=40)
    with pytest.raises(ValueError, match=r"runs.*popsize 4096 x 32.*160 KiB"):
        _call(sa, popsize=4096, n=32)


def test_vdcma_refuses_runs(sa):
    with pytest.raises(ValueError, match="runs"):
        sa.optimize.minimize(sa.factory.sphere, [[-3.0, 3.0]] * N, method="vdcma", options=dict(BASE))


def test_reference_checks_still_come_first(sa):
    """The reference's own argument checks (_evolution.check_arguments: cmaes/_cmaes.py:142-160) are not displaced by the new
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
        _call(sa, x0=np.zeros(N + 1))
    assert "runs" not in str(e.value)
    with pytest.raises(ValueError) as e:
        _call(sa, x0=np.zeros((2, 2, N)))
    assert "runs" not in str(e.value)


def test_runs_one_or_none_is_the_single_call(sa, monkeypatch):
    """runs=None and runs=1 take today's path: the batched front end is not entered."""
    from stochopy_amd.optimize import _cmaes

    class Entered(Exception):
        pass

    def boom(*a, **k):
        raise AssertionError("the batched front end was entered")

    def single(*a, **k):
        raise Entered

    monkeypatch.setattr(_cmaes, "_minimize_runs", boom)
    monkeypatch.setattr(_cmaes, "_CmaDeviceRun", single)
    for r in (None, 1):
        with pytest.raises(Entered):
            _call(sa, runs=r)


# ---- the plain generation-1 reference of tests/test_gpu_cma_runs_edges.py, validated against the oracle (no GPU)
GEN_CASES = [(obj, n, P) for n, P in _cma_runs_abi.GEN1_LITERALS for obj in ("sphere", "rosenbrock")] + \
            [("rosenbrock", 5, 12), ("rastrigin", 32, 64), ("sphere", 17, 172), ("sphere", 32, 432)]


@pytest.mark.parametrize("cfg", GEN_CASES, ids=lambda c: "%s_n%d_p%d" % c)
def test_generation_one_reference_agrees_with_the_oracle_probe(cfg):
    """_cma_runs_abi.generation_one is the oracle's generation 1 wherever the fitness values have no ties (with ties the
    oracle's default argsort is not the stable one): the same ranking, the mean within the bound of a mu-term sum in doubles
    (the oracle's np.dot) against the reference's long-double sum, the step size to a few ulp plus what that bound passes
    on through |ps| (a difference of two means, over sigma), x and
    fun exactly."""
    import oracle

    obj, n, P = cfg
    lower, upper = _cma_runs_abi.gen1_box(n)
    x0 = _cma_runs_abi.gen1_x0(n, 2)
    for r, seed in enumerate((700, 701)):
        ref = _cma_runs_abi.generation_one(obj, lower, upper, P, seed, x0[r], sigma=_cma_runs_abi.GEN1_SIGMA)
        if len(np.unique(ref["fit"])) < P:
            assert (obj, n) == ("rosenbrock", 1)  # an empty sum: every row is 0.0 (the one shape with ties)
            continue
        seen = []
        res = oracle.minimize(obj, np.transpose([lower, upper]), x0=x0[r], method="cmaes", rng="philox",
                              options={"maxiter": 1, "popsize": P, "seed": seed, "sigma": _cma_runs_abi.GEN1_SIGMA,
                                       "eigh": "canonical", "probe": lambda it, before, after: seen.append(after)})
        after, = seen
        assert np.array_equal(after["arx"], ref["arx"]) and np.array_equal(after["arfit"], ref["fit"])
        assert np.array_equal(after["order"], ref["order"])
        assert (np.abs(after["xmean"] - ref["xmean"]) <= ref["mu"] * 2.0 ** -53 * ref["absum"]).all()
        moved = np.linalg.norm(ref["mu"] * 2.0 ** -53 * ref["absum"])  # what the two means may differ by, through |ps|:
        assert abs(after["sigma"] - ref["sigma"]) <= ref["sigma_sens"] * moved + 8 * np.spacing(ref["sigma"])
        assert (res.nit, res.nfev, res.status) == (ref["nit"], ref["nfev"], ref["status"]) == (1, P, -1)
        assert np.array_equal(res.x, ref["x"]) and res.fun == ref["fun"]
