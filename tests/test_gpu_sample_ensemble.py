"""GPU: the affine-invariant ensemble sampler of stochopy_amd.sample (method="ensemble"; csrc/sx_sample_ensemble.hip: one
ensemble of walkers inside one workgroup's LDS, one launch per run; around a caller's objective a propose and a decide kernel per
half-sweep) against the numpy restatement (tests/_ensemble_oracle.py) at every sample, against itself under other launch
geometries, and against the rotated Gaussian it is meant to sample.  Tolerances are the sampler tests' (test_gpu_sample.py): 1e-6
of the search range for samples, 1e-6 relative for values; counts are exact.  Seeds are admitted by the restatement alone
(_ensemble_cases.admitted)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _ensemble_cases as cases  # noqa: E402
import _ensemble_oracle  # noqa: E402
from _sample_metric_cases import GAUSS_BOUNDS, SIGMA  # noqa: E402
from test_gpu_sample_batched import device_objective  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sa():
    import stochopy_amd

    return stochopy_amd


def close_samples(got, want, span):
    return np.allclose(got, want, rtol=0, atol=1e-6 * span, equal_nan=True)


def close_values(got, want):
    return np.allclose(got, want, rtol=1e-6, atol=0, equal_nan=True)


def run(sa, fun, bounds, x0=None, args=(), callback=None, **options):
    return sa.sample.sample(fun, bounds, x0=x0, args=args, method="ensemble", callback=callback,
                            options=dict(options, rng="philox", backend="hip"))


def check_against(got, want, Cn, W, m, n, span, reject):
    assert got.nit == want.nit == m and got.walkers == W == want.walkers and got.stretch == want.stretch
    assert got.xall.shape == ((Cn, m, W, n) if Cn > 1 else (m, W, n)) and got.funall.shape == got.xall.shape[:-1]
    assert got.accept_ratios.shape == (Cn, W)
    with np.errstate(all="ignore"):
        print("    max |dx| / range", np.nanmax(np.abs(got.xall - want.xall)) / span, "accepted", int(want.nacc.sum()), "of",
              Cn * W * (m - 1), "infeasible", int(Cn * W * (m - 1) - want.nfeas.sum()))
    assert np.array_equal(got.accept_ratios, want.accept_ratios)  # nacc / maxiter: the counts, exactly
    assert got.accept_ratio == want.accept_ratio
    if reject:
        assert got.nreject == want.nreject
    else:
        assert "nreject" not in got
    assert close_samples(got.xall, want.xall, span) and close_values(got.funall, want.funall)
    assert close_samples(got.x, want.x, span) and close_values(got.fun, want.fun)


# (objective, ndim, W, ensembles, constraints, stretch, x0, half-width of the box)
#   ndim 1 / 2 / 8; 16 / 17 / 33: the e / e + LPR boundary of a 16-lane row, more than one element per lane; 64: the 16-lane
#   limit; 65 / 96: 32 lanes.  W = 2 ndim except (8, 16 -> h = 8: two wavefronts) and (16, 40): h = 20 over 16 row groups, two
#   passes, the second ragged; (2, 6): h = 3, a wavefront with an idle row group; (64, 128): 74 KiB of LDS, (96, 192): the largest
#   (ndim, 2 ndim) sx_sample_ensemble_lds_bytes admits (158.5 of 160 KiB), six passes.
#   "Reject" with stretch 1.5 / 3 in a box so small that the objective is nearly flat over it: the walkers stay spread and most
#   proposals leave.
SHAPES = [
    ("sphere", 1, 4, 1, None, 2.0, None, 5.12),
    ("rosenbrock", 2, 6, 7, None, 2.0, "shared", 5.12),
    ("rastrigin", 8, 16, 5, "Reject", 3.0, None, 0.05),
    ("sphere", 16, 40, 3, None, 2.0, "per-ensemble", 5.12),
    ("rosenbrock", 17, 34, 2, None, 2.0, "per-ensemble", 5.12),
    ("styblinski_tang", 33, 66, 3, "Reject", 1.5, None, 0.1),
    ("sphere", 64, 128, 2, None, 2.0, "shared", 5.12),
    ("rastrigin", 65, 130, 2, None, 2.0, None, 5.12),
    ("sphere", 96, 192, 2, None, 2.0, None, 5.12),
]


@pytest.mark.parametrize("objective,ndim,W,Cn,constraints,stretch,x0,half", SHAPES,
                         ids=[f"{s[0]}-n{s[1]}-W{s[2]}-C{s[3]}" for s in SHAPES])
def test_parity_with_the_restatement_at_every_sample(sa, objective, ndim, W, Cn, constraints, stretch, x0, half):
    from stochopy_amd import _lib

    L = _lib.lib()
    if ndim == 96:
        assert 0 < L.sx_sample_ensemble_lds_bytes(192, 96) <= 160 * 1024 < L.sx_sample_ensemble_lds_bytes(194, 97)
    if ndim == 64:
        assert L.sx_sample_ensemble_lds_bytes(W, ndim) > 64 * 1024
    bounds = [[-half, half]] * ndim
    span = 2.0 * half
    rs = np.random.RandomState(ndim + W)
    start = {None: None, "shared": rs.uniform(-2.0, 2.0, (W, ndim)), "per-ensemble": rs.uniform(-2.0, 2.0, (Cn, W, ndim))}[x0]
    base = {"maxiter": 30, "walkers": W, "stretch": stretch, "constraints": constraints, "chains": Cn, "seed": 700 + ndim}
    seed, want30 = cases.admitted(objective, bounds, start, base)
    for m in (1, 2, 30):
        o = dict(base, maxiter=m, seed=seed)
        print(f"  maxiter {m} seed {seed}")
        with np.errstate(all="ignore"):
            want = want30 if m == 30 else _ensemble_oracle.sample(objective, bounds, x0=start, options=dict(o))
        got = run(sa, getattr(sa.factory, objective), bounds, x0=start, **o)
        check_against(got, want, Cn, W, m, ndim, span, constraints == "Reject")
    total = Cn * W * 29
    assert 0 < want30.nacc.sum() < total  # both outcomes of the decision
    if constraints == "Reject":
        assert want30.nfeas.sum() < total // 2  # most proposals leave the box
        assert np.all(np.abs(got.xall) <= half)


@pytest.mark.parametrize("ndim,W", [(3, 8), (16, 40), (65, 130)])
def test_an_ensemble_does_not_depend_on_its_neighbours_or_the_launches(sa, ndim, W):
    """Ensemble 2 is ensemble 2 among 3 ensembles or among 50, a run cut into one launch per sample by a callback is the run in
    one launch, and a run repeated is the same run -- all bit for bit; the callback's states are the restatement's."""
    bounds = [[-5.12, 5.12]] * ndim
    m = 20
    o = {"maxiter": m, "walkers": W, "seed": 9}
    seed, want = cases.admitted("rastrigin", bounds, None, dict(o, chains=3))
    o["seed"] = seed
    fun = sa.factory.rastrigin
    few = run(sa, fun, bounds, chains=3, **o)
    many = run(sa, fun, bounds, chains=50, **o)
    again = run(sa, fun, bounds, chains=3, **o)
    assert 0.0 < few.accept_ratio < 1.0 and np.all(np.isfinite(few.funall))
    for key in ("xall", "funall", "accept_ratios"):
        assert np.array_equal(few[key], many[key][:3]), key
        assert np.array_equal(few[key], again[key]), key
    seen, told = [], []
    cut = run(sa, fun, bounds, chains=3, **o,
              callback=lambda xk, state: seen.append((np.array(xk, copy=True), state.nit, state.fun, np.array(state.x),
                                                      state.accept_ratio, state.xall.shape)))
    assert len(seen) == m and np.array_equal(np.stack([s[0] for s in seen], axis=1), few.xall)
    assert [s[1] for s in seen] == list(range(1, m + 1))
    for key in ("xall", "funall", "accept_ratios", "x", "fun", "accept_ratio"):
        assert np.array_equal(cut[key], few[key]), key
    with np.errstate(all="ignore"):
        _ensemble_oracle.sample("rastrigin", bounds, options=dict(o, chains=3),
                                callback=lambda xk, state: told.append((xk, state.nit, state.fun, state.x, state.accept_ratio,
                                                                        state.xall.shape)))
    for got, ref in zip(seen, told):
        assert close_samples(got[0], ref[0], 10.24) and got[1] == ref[1] and close_values(got[2], ref[2])
        assert close_samples(got[3], ref[3], 10.24) and got[4] == ref[4] and got[5] == ref[5]
    check_against(few, want, 3, W, m, ndim, 10.24, False)


@pytest.mark.parametrize("objective,ndim,W,Cn,constraints,return_all", [
    ("rastrigin", 3, 8, 7, None, True), ("sphere", 16, 40, 3, None, True), ("styblinski_tang", 70, 140, 2, None, True),
    ("rosenbrock", 5, 12, 20, "Reject", False)])
def test_a_callers_objective_gives_the_resident_run(sa, objective, ndim, W, Cn, constraints, return_all):
    """factory.batched of a function that returns sx_eval's values: propose -> fun -> decide per half-sweep is the resident run,
    bit for bit ((16, 40): the resident run walks each half in two passes)."""
    half = 1.0 if constraints else 5.12
    bounds = [[-half, half]] * ndim
    o = {"maxiter": 25, "walkers": W, "chains": Cn, "seed": 40 + ndim, "constraints": constraints, "return_all": return_all}
    fused = run(sa, getattr(sa.factory, objective), bounds, **o)
    ext = run(sa, device_objective(sa, objective), bounds, **o)
    assert ("xall" in fused) == return_all == ("xall" in ext)
    for key in ("x", "fun", "accept_ratio", "accept_ratios") + (("xall", "funall") if return_all else ()) + \
            (("nreject",) if constraints else ()):
        assert np.array_equal(ext[key], fused[key]), key
    assert 0.0 < fused.accept_ratio < 1.0
    if constraints:
        assert fused.nreject > 0
    if return_all:
        assert np.all(np.isfinite(fused.funall))
        seen = []
        cut = run(sa, device_objective(sa, objective), bounds, **o, callback=lambda xk, state: seen.append(np.array(xk, copy=True)))
        assert np.array_equal(cut.xall, fused.xall) and np.array_equal(np.stack(seen, axis=1), fused.xall)


def test_a_torch_objective_beyond_the_lds_limit_agrees_with_the_restatement(sa):
    """ndim 129: rows of 64 lanes, W = 258 -- no resident form; the walkers live in device memory."""
    import torch

    ndim, W, Cn, m = 129, 258, 2, 12
    bounds = [[-5.12, 5.12]] * ndim
    centre = np.linspace(-1.0, 1.0, ndim)
    base = {"maxiter": m, "walkers": W, "chains": Cn, "seed": 66}
    seed, want = cases.admitted(lambda X: (0.7 * (X - centre) ** 2).sum(axis=1), bounds, None, base)
    fun = sa.factory.batched(lambda X, c, s: (s * (X - c) ** 2).sum(dim=1))
    got = run(sa, fun, bounds, args=(torch.tensor(centre, device="cuda"), 0.7), **dict(base, seed=seed))
    check_against(got, want, Cn, W, m, ndim, 10.24, False)
    assert 0 < want.nacc.sum() < Cn * W * (m - 1)
    with pytest.raises(ValueError, match="walkers"):
        run(sa, sa.factory.sphere, bounds, **base)


def test_nan_inf_and_ties_follow_the_restatement(sa):
    """A caller's objective that plants them: the value is floor(2 |x0|) (exact ties), NaN where x1 > 1.5, +inf where
    x1 < -1.5 -- single correctly rounded operations, the same bits in torch and numpy.  A NaN d accepts, inf - inf is NaN, inf
    against a finite value never wins."""
    import torch

    def planted(X):
        f = torch.floor(2.0 * torch.abs(X[:, 0]))
        f = torch.where(X[:, 1] > 1.5, torch.full_like(f, float("nan")), f)
        return torch.where(X[:, 1] < -1.5, torch.full_like(f, float("inf")), f)

    def planted_np(X):
        f = np.floor(2.0 * np.abs(X[:, 0]))
        f = np.where(X[:, 1] > 1.5, np.nan, f)
        return np.where(X[:, 1] < -1.5, np.inf, f)

    Cn, W, m = 40, 6, 40
    bounds = [[-5.12, 5.12]] * 2
    o = {"maxiter": m, "walkers": W, "chains": Cn, "seed": 3}
    with np.errstate(all="ignore"):
        want = _ensemble_oracle.sample(planted_np, bounds, options=dict(o))
    got = run(sa, sa.factory.batched(planted), bounds, **o)
    f = want.funall
    print("samples: NaN", int(np.isnan(f).sum()), "inf", int(np.isinf(f).sum()), "ties with the previous sample",
          int((f[:, 1:] == f[:, :-1]).sum()))
    assert np.isnan(f).any() and np.isinf(f).any() and np.isfinite(f).any()
    assert np.array_equal(np.isnan(got.funall), np.isnan(f)) and np.array_equal(np.isinf(got.funall), np.isinf(f))
    check_against(got, want, Cn, W, m, 2, 10.24, False)


def test_it_samples_the_rotated_gaussian_on_the_device(sa):
    """tests/test_sample_ensemble_host.py's rotated target through factory.batched with 256 ensembles of 16 walkers: the
    per-axis variance over sigma^2 in the rotated frame stays within the host test's bound (the yardstick is the Gaussian, not
    the device)."""
    import torch

    Q = torch.tensor(cases.ROTATION, device="cuda")
    sigma = torch.tensor(SIGMA, device="cuda")
    fun = sa.factory.batched(lambda X: 0.5 * (((X @ Q) / sigma) ** 2).sum(dim=1))
    got = run(sa, fun, GAUSS_BOUNDS, **cases.options(2024, chains=256))
    r = cases.variance_ratio(got.xall, cases.ROTATION)
    print("variance / sigma^2", r.min(), "..", r.max(), "accept_ratio", got.accept_ratio, "bound", cases.BOUND)
    assert np.all(np.abs(r - 1.0) <= cases.BOUND)
    assert 0.3 < got.accept_ratio < 0.6


def test_the_result_object(sa):
    bounds = [[-5.12, 5.12]] * 3
    o = {"maxiter": 30, "seed": 4}
    want = _ensemble_oracle.sample("sphere", bounds, options=dict(o, chains=6))
    many = run(sa, sa.factory.sphere, bounds, chains=6, **o)
    one = run(sa, sa.factory.sphere, bounds, chains=1, **o)
    bare = run(sa, sa.factory.sphere, bounds, chains=6, return_all=False, **o)
    direct = sa.sample.ensemble(sa.factory.sphere, bounds, chains=6, **o)
    assert many.walkers == 6 and many.stretch == 2.0  # walkers=None: max(4, 2 ndim)
    assert many.xall.shape == (6, 30, 6, 3) and many.funall.shape == (6, 30, 6) and many.x.shape == (3,)
    assert one.xall.shape == (30, 6, 3) and one.funall.shape == (30, 6) and one.accept_ratios.shape == (1, 6)
    assert np.array_equal(one.xall, many.xall[0])  # ensemble 0 alone is ensemble 0
    assert "xall" not in bare and "funall" not in bare and np.array_equal(bare.accept_ratios, many.accept_ratios)
    assert bare.fun == many.fun and np.array_equal(bare.x, many.x)
    assert np.array_equal(direct.xall, many.xall)
    for res in (many, one, bare):
        assert res.nit == 30 and "nreject" not in res
    assert many.accept_ratio == want.accept_ratio == want.nacc.sum() / (6 * 6 * 30)
    assert close_values(many.fun, want.fun) and close_samples(many.x, want.x, 10.24)  # the best accepted sample of any walker
    f = many.funall.reshape(6, 30, 6)
    assert many.fun == min(f[g, it, w] for g in range(6) for it in range(1, 30) for w in range(6) if f[g, it, w] != f[g, it - 1, w])
