"""GPU: parallel tempering for stochopy_amd.sample (csrc/sx_sample_temper.hip: ladders of device-resident replicas, one
ladder inside one workgroup; around a caller's objective csrc/sx_sample_unfused.hip) against the numpy restatement
(tests/_temper_oracle.py) at every sample, against the plain chain kernel, against itself under other launch geometries, and
against the multimodal distribution it is meant to sample.  Tolerances are the sampler tests' (test_gpu_sample.py): 1e-6 of
the search range for samples, 1e-6 relative for values; counts are exact."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _temper_oracle  # noqa: E402
from oracle import objectives  # noqa: E402
from test_gpu_sample_batched import device_objective  # noqa: E402
from test_sample_temper_host import TARGET, cold_share, rastrigin_mass  # noqa: E402

pytestmark = pytest.mark.gpu

SPAN = 10.24


@pytest.fixture(scope="module")
def sa():
    import stochopy_amd

    return stochopy_amd


def close_samples(got, want):
    return np.allclose(got, want, rtol=0, atol=1e-6 * SPAN, equal_nan=True)


def close_values(got, want):
    return np.allclose(got, want, rtol=1e-6, atol=0, equal_nan=True)


def admitted(fun, bounds, ladder, x0, opts, tries=8):
    """A parity tolerance only means something where the restatement's own rounding stays well inside it
    (tools/sample_sensitivity.py): the first seed from opts["seed"] on whose restated run keeps every count and stays within
    1e-9 when each objective value is moved at random by one unit in the last place.  The restatement alone decides."""
    f = objectives.OBJECTIVES[fun] if isinstance(fun, str) else fun
    rs = np.random.RandomState(0)

    def moved(X):
        v = np.asarray(f(X), dtype=np.float64)
        return np.nextafter(v, v + rs.choice([-1.0, 1.0], size=v.shape))

    for seed in range(opts["seed"], opts["seed"] + tries):
        o = dict(opts, seed=seed)
        with np.errstate(all="ignore"):
            a = _temper_oracle.sample(f, bounds, ladder, x0=x0, options=dict(o))
            b = _temper_oracle.sample(moved, bounds, ladder, x0=x0, options=dict(o))
            same = all(np.array_equal(a[key], b[key]) for key in ("nacc", "nfeas", "nswap"))
            if same and np.nanmax(np.abs(a.xall - b.xall)) <= 1e-9 * SPAN and close_values(a.funall, b.funall):
                return seed, a
    raise AssertionError("no admissible seed")


def check_against(got, want, Cn, K, m, n, reject):
    assert got.nit == want.nit == m
    assert got.xall.shape == ((Cn, m, n) if Cn > 1 else (m, n)) and got.funall.shape == got.xall.shape[:-1]
    assert got.accept_ratios.shape == (Cn, K) and got.swap_ratios.shape == (Cn, K - 1)
    with np.errstate(all="ignore"):
        print("    max |dx| / range", np.nanmax(np.abs(got.xall - want.xall)) / SPAN, "accepted", int(want.nacc.sum()),
              "of", Cn * K * (m - 1), "exchanges", int(want.nswap.sum()), "infeasible",
              int(Cn * K * (m - 1) - want.nfeas.sum()))
    assert np.array_equal(got.accept_ratios, want.accept_ratios)  # nacc / maxiter: the counts, exactly
    assert np.array_equal(got.swap_ratios, want.swap_ratios)
    assert got.accept_ratio == want.accept_ratio
    if reject:
        assert got.nreject == want.nreject
    assert close_samples(got.xall, want.xall) and close_values(got.funall, want.funall)
    assert close_samples(got.x, want.x) and close_values(got.fun, want.fun)


# (objective, ndim, K, ladders, perc, constraints, stepsize, x0)
#   ndim 1 / 2 / 16 / 17 / 33: one lane pair, the e / e + LPR boundary of a 16-lane row, more than one pair per lane;
#   100: 32 lanes; 129 / 300 / 2048: 64 lanes (one row per wavefront, 8 rows per workgroup)
#   K = 2; K = 3 / 5: the top rung sits out at odd events and 16 = 5 * 3 + 1 = 3 * 5 + 1 rows leave one over (ndim 129, K = 3:
#   8 = 2 * 3 + 2); K = 16 at ndim <= 128; K = sx_sample_tempered_max_rungs: 8 at ndim 129, 4 at 2 048 (132 KB of LDS: the
#   launch raises the kernel's limit); ladders such that the replicas span several workgroups and the last one is ragged
SHAPES = [
    ("sphere", 1, 2, 1, 1.0, None, 0.05, None),
    ("rosenbrock", 2, 3, 7, 1.0, None, 0.05, "shared"),
    ("rastrigin", 16, 5, 40, 1.0, None, 0.05, "per-ladder"),
    ("sphere", 17, 16, 3, 0.3, None, 0.05, None),
    ("rosenbrock", 33, 2, 33, 0.5, "Reject", 0.5, None),
    ("sphere", 8, 5, 9, 1.0, "Reject", 0.5, "per-ladder"),
    ("rastrigin", 100, 16, 2, 0.3, None, 0.02, "shared"),
    ("sphere", 129, 3, 5, 1.0, None, 0.02, None),
    ("rosenbrock", 129, 8, 3, 0.3, None, 0.02, "per-ladder"),
    ("rastrigin", 300, 5, 3, 0.3, None, 0.02, None),
    ("sphere", 2048, 4, 3, 0.3, None, 0.005, None),
]


@pytest.mark.parametrize("objective,ndim,K,Cn,perc,constraints,stepsize,x0", SHAPES,
                         ids=[f"{s[0]}-n{s[1]}-K{s[2]}-C{s[3]}" for s in SHAPES])
def test_parity_with_the_restatement_at_every_sample(sa, objective, ndim, K, Cn, perc, constraints, stepsize, x0):
    from stochopy_amd import _lib

    if (ndim, K) in ((129, 8), (2048, 4)):
        assert _lib.lib().sx_sample_tempered_max_rungs(ndim) == K
    bounds = [[-5.12, 5.12]] * ndim
    ladder = np.geomspace(1.0, 20.0, K)
    rs = np.random.RandomState(ndim + K)
    start = {None: None, "shared": rs.uniform(-2.0, 2.0, ndim), "per-ladder": rs.uniform(-2.0, 2.0, (Cn, ndim))}[x0]
    if x0 == "per-ladder" and Cn == 1:
        start = start[0]
    for every in (1, 3, 1000):
        base = {"maxiter": 40, "stepsize": stepsize, "perc": perc, "constraints": constraints, "chains": Cn,
                "swap_every": every, "seed": 500 + ndim + K}
        seed, want40 = admitted(objective, bounds, ladder, start, base)
        for m in (1, 2, 40):
            o = dict(base, maxiter=m, seed=seed)
            print(f"  swap_every {every} maxiter {m} seed {seed}")
            with np.errstate(all="ignore"):
                want = want40 if m == 40 else _temper_oracle.sample(objective, bounds, ladder, x0=start, options=dict(o))
            got = sa.sample.sample(getattr(sa.factory, objective), bounds, x0=start, method="mcmc",
                                   options=dict(o, temperatures=ladder, rng="philox", backend="hip"))
            check_against(got, want, Cn, K, m, ndim, constraints == "Reject")
            assert np.array_equal(got.temperatures, ladder)
        if every == 1:
            assert want40.nswap.sum() > 0 and 0 < want40.nacc.sum() < Cn * K * 39  # both outcomes of both decisions
        if constraints == "Reject":
            assert want40.nfeas.sum() < Cn * K * 39  # proposals do leave the box


@pytest.mark.parametrize("objective,ndim,K,Cn,perc", [("rastrigin", 3, 5, 7, 1.0), ("styblinski_tang", 130, 8, 5, 0.3),
                                                      ("sphere", 64, 16, 3, 0.5)])
def test_without_events_the_cold_rung_is_the_plain_chain(sa, objective, ndim, K, Cn, perc):
    """swap_every > maxiter: rung 0 of ladder c is chain c K of the plain run with C K chains (csrc/sx_sample.hip), bit for
    bit -- beta[0] = 1.0 leaves the cold rung's rule what it is, the replica index is the chain index."""
    bounds = [[-5.12, 5.12]] * ndim
    o = {"maxiter": 40, "stepsize": 0.05, "perc": perc, "seed": 21, "rng": "philox", "backend": "hip"}
    got = sa.sample.sample(getattr(sa.factory, objective), bounds, method="mcmc",
                           options=dict(o, chains=Cn, temperatures=np.geomspace(1.0, 9.0, K), swap_every=41))
    plain = sa.sample.sample(getattr(sa.factory, objective), bounds, method="mcmc", options=dict(o, chains=Cn * K))
    assert np.all(np.isfinite(plain.funall))
    assert np.array_equal(got.xall, plain.xall[::K]) and np.array_equal(got.funall, plain.funall[::K])
    assert np.array_equal(got.accept_ratios[:, 0], plain.accept_ratios[::K])
    assert 0.0 < got.accept_ratio < 1.0 and np.all(got.swap_ratios == 0.0)


@pytest.mark.parametrize("ndim,K,every", [(8, 5, 1), (130, 3, 2), (40, 16, 3)])
def test_a_ladder_does_not_depend_on_its_neighbours(sa, ndim, K, every):
    """Ladder 2 is ladder 2 among 3 ladders or among 50 (other workgroups, other slots in them), a run cut into one launch per
    sample by a callback is the run in one launch, and a run repeated is the same run -- all bit for bit."""
    bounds = [[-5.12, 5.12]] * ndim
    o = {"maxiter": 40, "stepsize": 0.05, "seed": 9, "rng": "philox", "backend": "hip", "swap_every": every,
         "temperatures": np.geomspace(1.0, 16.0, K)}
    fun = sa.factory.rastrigin
    few = sa.sample.sample(fun, bounds, method="mcmc", options=dict(o, chains=3))
    many = sa.sample.sample(fun, bounds, method="mcmc", options=dict(o, chains=50))
    again = sa.sample.sample(fun, bounds, method="mcmc", options=dict(o, chains=3))
    assert few.swap_ratios.max() > 0.0 and np.all(np.isfinite(few.funall))
    for key in ("xall", "funall", "accept_ratios", "swap_ratios"):
        assert np.array_equal(few[key], many[key][:3]), key
        assert np.array_equal(few[key], again[key]), key
    seen = []
    cut = sa.sample.sample(fun, bounds, method="mcmc", options=dict(o, chains=3),
                           callback=lambda xk, state: seen.append((np.array(xk, copy=True), state.nit, state.fun)))
    assert len(seen) == 40 and np.array_equal(np.stack([s[0] for s in seen], axis=1), few.xall)
    assert [s[1] for s in seen] == list(range(1, 41)) and seen[-1][2] == few.fun
    for key in ("xall", "funall", "accept_ratios", "swap_ratios", "x", "fun", "accept_ratio"):
        assert np.array_equal(cut[key], few[key]), key


@pytest.mark.parametrize("objective,ndim,K,Cn,every,return_all", [
    ("rastrigin", 3, 3, 7, 1, True), ("styblinski_tang", 130, 5, 4, 3, True), ("sphere", 2048, 4, 2, 2, True),
    ("rastrigin", 17, 2, 20, 1, False), ("sphere", 33, 16, 3, 2, True)])
def test_a_callers_objective_gives_the_resident_run(sa, objective, ndim, K, Cn, every, return_all):
    """factory.batched of a function that returns sx_eval's values: propose -> fun -> decide -> swap kernel is the resident
    tempered run, bit for bit (K = 2 at an even event launches no swap kernel; an odd event hands row `it` of xall to it)."""
    bounds = [[-5.12, 5.12]] * ndim
    o = {"maxiter": 12 if ndim > 1000 else 30, "stepsize": 0.05, "perc": 0.5, "seed": 40 + ndim, "rng": "philox",
         "backend": "hip", "chains": Cn, "temperatures": np.geomspace(1.0, 12.0, K), "swap_every": every,
         "return_all": return_all}
    fused = sa.sample.sample(getattr(sa.factory, objective), bounds, method="mcmc", options=dict(o))
    ext = sa.sample.sample(device_objective(sa, objective), bounds, method="mcmc", options=dict(o))
    assert ("xall" in fused) == return_all == ("xall" in ext)
    for key in ("x", "fun", "accept_ratio", "accept_ratios", "swap_ratios", "temperatures") + (("xall", "funall") if return_all else ()):
        assert np.array_equal(ext[key], fused[key]), key
    assert fused.swap_ratios.max() > 0.0
    if return_all:
        assert np.all(np.isfinite(fused.funall))
        seen = []
        cut = sa.sample.sample(device_objective(sa, objective), bounds, method="mcmc", options=dict(o),
                               callback=lambda xk, state: seen.append(np.array(xk, copy=True)))
        assert np.array_equal(cut.xall, fused.xall) and np.array_equal(cut.swap_ratios, fused.swap_ratios)
        assert np.array_equal(np.stack(seen, axis=-2), fused.xall)


def test_a_torch_objective_with_args_agrees_with_the_restatement(sa):
    import torch

    ndim, K, Cn = 6, 4, 9
    bounds = [[-5.12, 5.12]] * ndim
    centre, scale = np.linspace(-1.0, 1.0, ndim), 0.7
    fun = sa.factory.batched(lambda X, c, s: (s * (X - c) ** 2).sum(dim=1))
    ladder = np.geomspace(1.0, 8.0, K)
    base = {"maxiter": 40, "stepsize": 0.1, "chains": Cn, "swap_every": 2, "seed": 66}
    seed, want = admitted(lambda X: (scale * (X - centre) ** 2).sum(axis=1), bounds, ladder, None, base)
    got = sa.sample.sample(fun, bounds, args=(torch.tensor(centre, device="cuda"), scale), method="mcmc",
                           options=dict(base, seed=seed, temperatures=ladder, rng="philox", backend="hip"))
    check_against(got, want, Cn, K, 40, ndim, False)
    assert want.nswap.sum() > 0


def test_a_wrong_objective_raises_at_the_first_call(sa):
    """... and leaves the process usable: the next run is served."""
    bounds = [[-5.12, 5.12]] * 4
    o = {"maxiter": 5, "chains": 3, "seed": 1, "rng": "philox", "temperatures": [1.0, 2.0]}
    with pytest.raises(ValueError):
        sa.sample.sample(sa.factory.batched(lambda X: X.sum(dim=1)[:-1]), bounds, method="mcmc", options=dict(o))
    with pytest.raises(TypeError):
        sa.sample.sample(sa.factory.batched(lambda X: X.sum(dim=1).cpu()), bounds, method="mcmc", options=dict(o))
    ok = sa.sample.sample(sa.factory.batched(lambda X: (X * X).sum(dim=1)), bounds, method="mcmc", options=dict(o))
    assert ok.xall.shape == (3, 5, 4) and np.all(np.isfinite(ok.funall))


def test_nan_inf_and_ties_follow_the_restatement(sa):
    """A caller's objective that plants them: the value is floor(2 |x0|) (exact ties between neighbours), NaN where
    x1 > 1.5, +inf where x1 < -1.5 -- single correctly rounded operations, the same bits in torch and numpy.  A NaN d accepts
    and exchanges, inf - inf is NaN, inf against a finite value never wins."""
    import torch

    def planted(X):
        f = torch.floor(2.0 * torch.abs(X[:, 0]))
        f = torch.where(X[:, 1] > 1.5, torch.full_like(f, float("nan")), f)
        return torch.where(X[:, 1] < -1.5, torch.full_like(f, float("inf")), f)

    def planted_np(X):
        f = np.floor(2.0 * np.abs(X[:, 0]))
        f = np.where(X[:, 1] > 1.5, np.nan, f)
        return np.where(X[:, 1] < -1.5, np.inf, f)

    Cn, K, m = 40, 5, 40
    bounds = [[-5.12, 5.12]] * 2
    ladder = np.geomspace(1.0, 10.0, K)
    o = {"maxiter": m, "stepsize": 0.1, "chains": Cn, "swap_every": 1, "seed": 3}
    with np.errstate(all="ignore"):
        want = _temper_oracle.sample(planted_np, bounds, ladder, options=dict(o), keep_hot=True)
    got = sa.sample.sample(sa.factory.batched(planted), bounds, method="mcmc",
                           options=dict(o, temperatures=ladder, rng="philox", backend="hip"))
    f = want.funall
    print("cold samples: NaN", int(np.isnan(f).sum()), "inf", int(np.isinf(f).sum()), "ties with the previous sample",
          int((f[:, 1:] == f[:, :-1]).sum()), "exchanges", int(want.nswap.sum()))
    assert np.isnan(f).any() and np.isinf(f).any() and np.isfinite(f).any()
    assert np.array_equal(np.isnan(got.funall), np.isnan(f)) and np.array_equal(np.isinf(got.funall), np.isinf(f))
    check_against(got, want, Cn, K, m, 2, False)


def test_it_samples_a_multimodal_target(sa):
    """tests/test_sample_temper_host.py's 1-D rastrigin case on the resident path with 1 024 ladders of 8: the cold rungs'
    share of samples in the central well is the exact mass within 0.03 (the bound of the host test; the yardstick is the
    quadrature, not the device), every pair exchanges at a rate in (0.3, 1), and the plain run never leaves x = 3's well."""
    want = rastrigin_mass()
    o = dict(TARGET["options"], seed=2024, chains=1024, rng="philox", backend="hip")
    got = sa.sample.sample(sa.factory.rastrigin, TARGET["bounds"], x0=TARGET["x0"], method="mcmc",
                           options=dict(o, temperatures=TARGET["ladder"]))
    share = cold_share(got.xall)
    print("share", share, "exact", want, "swap ratios", got.swap_ratios.min(), "..", got.swap_ratios.max())
    assert abs(share - want) <= 0.03
    assert np.all(got.swap_ratios > 0.3) and np.all(got.swap_ratios < 1.0)
    assert np.all(np.abs(got.xall) <= 5.12)
    o.pop("swap_every")
    plain = sa.sample.sample(sa.factory.rastrigin, TARGET["bounds"], x0=TARGET["x0"], method="mcmc", options=o)
    assert cold_share(plain.xall) == 0.0


def test_the_result_object(sa):
    bounds = [[-5.12, 5.12]] * 3
    ladder = [1.0, 2.0, 5.0, 11.0]
    o = {"maxiter": 30, "seed": 4, "rng": "philox", "temperatures": ladder, "swap_every": 4, "stepsize": 0.05}
    want = _temper_oracle.sample("sphere", bounds, ladder, options={"maxiter": 30, "seed": 4, "swap_every": 4,
                                                                    "stepsize": 0.05, "chains": 6})
    many = sa.sample.sample(sa.factory.sphere, bounds, method="mcmc", options=dict(o, chains=6))
    one = sa.sample.sample(sa.factory.sphere, bounds, method="mcmc", options=dict(o, chains=1))
    bare = sa.sample.sample(sa.factory.sphere, bounds, method="mcmc", options=dict(o, chains=6, return_all=False))
    assert many.xall.shape == (6, 30, 3) and many.funall.shape == (6, 30) and many.x.shape == (3,)
    assert one.xall.shape == (30, 3) and one.funall.shape == (30,)  # squeezed as the plain run's
    assert one.accept_ratios.shape == (1, 4) and one.swap_ratios.shape == (1, 3)
    assert "xall" not in bare and "funall" not in bare and np.array_equal(bare.swap_ratios, many.swap_ratios)
    assert bare.fun == many.fun and np.array_equal(bare.x, many.x)
    for res in (many, one, bare):
        assert res.nit == 30 and res.temperatures.dtype == np.float64 and np.array_equal(res.temperatures, ladder)
        assert "nreject" not in res
    # events j = 1 .. 7 after samples 4, 8, ..., 28: pairs (0,1) and (2,3) at the four odd ones, (1,2) at the three even ones
    attempts = np.zeros(3, dtype=np.int64)
    for it in range(1, 30):
        if it % 4 == 0:
            j = it // 4
            for k in range(0 if j % 2 else 1, 3, 2):
                attempts[k] += 1
    assert attempts.tolist() == [4, 3, 4]
    assert np.array_equal(many.swap_ratios, want.nswap / attempts) and want.nswap.sum() > 0
    assert np.array_equal(one.swap_ratios, want.nswap[:1] / attempts)  # ladder 0 alone is ladder 0
    assert close_values(many.fun, want.fun) and close_samples(many.x, want.x)  # the best accepted or arrived cold sample
