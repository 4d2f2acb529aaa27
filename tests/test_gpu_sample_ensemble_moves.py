"""GPU: the moves of the ensemble sampler (method="ensemble" with ``moves`` / ``burn`` / ``thin``;
csrc/sx_sample_ensemble_moves.hip: one ensemble inside one workgroup's LDS, one launch per run; around a caller's objective a
propose and a decide kernel per half-sweep) against the numpy restatement (tests/_ensemble_moves_oracle.py) at every sample,
against the stretch-only entry points, against itself under other launch geometries, and on the bimodal target the moves are
for.  Tolerances: 1e-9 of the search range for samples, 1e-6 relative for values; counts are exact.  Seeds are admitted by the
restatement alone (_ensemble_moves_cases.admitted)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _ensemble_moves_cases as cases  # noqa: E402
import _ensemble_moves_oracle as oracle  # noqa: E402
from test_gpu_sample_batched import device_objective  # noqa: E402

pytestmark = pytest.mark.gpu

FOUR = [("stretch", 0.25), ("de", 0.25), ("de", 0.25, 1.0), ("snooker", 0.25)]  # every kind, and "de" at both of its gammas


@pytest.fixture(scope="module")
def sa():
    import stochopy_amd

    return stochopy_amd


def close_samples(got, want, span):
    return np.allclose(got, want, rtol=0, atol=1e-9 * span, equal_nan=True)


def close_values(got, want):
    return np.allclose(got, want, rtol=1e-6, atol=0, equal_nan=True)


def run(sa, fun, bounds, x0=None, args=(), callback=None, **options):
    return sa.sample.sample(fun, bounds, x0=x0, args=args, method="ensemble", callback=callback,
                            options=dict(options, rng="philox", backend="hip"))


def check_against(got, want, Cn, W, rows, n, span, reject):
    assert got.nit == want.nit and got.walkers == W == want.walkers
    assert got.moves == want.moves and (got.burn, got.thin) == (want.burn, want.thin)
    assert got.xall.shape == ((Cn, rows, W, n) if Cn > 1 else (rows, W, n)) and got.funall.shape == got.xall.shape[:-1]
    assert got.accept_ratios.shape == (Cn, W)
    with np.errstate(all="ignore"):
        print("    max |dx| / range", np.nanmax(np.abs(got.xall - want.xall)) / span, "accepted", int(want.nacc.sum()), "of",
              Cn * W * (want.nit - 1), "infeasible", int(Cn * W * (want.nit - 1) - want.nfeas.sum()))
    assert np.array_equal(got.accept_ratios, want.accept_ratios)  # nacc / maxiter: the counts, exactly
    assert got.accept_ratio == want.accept_ratio
    if reject:
        assert got.nreject == want.nreject
    else:
        assert "nreject" not in got
    assert close_samples(got.xall, want.xall, span) and close_values(got.funall, want.funall)
    assert close_samples(got.x, want.x, span) and close_values(got.fun, want.fun)


# (objective, ndim, W, ensembles, constraints, x0, half-width of the box)
#   (1, 4): h = 2, j2 is forced, "de" only; (1, 6): h = 3, every snooker triple is the whole half; (2, 6): a wavefront with an idle
#   row group; (8, 16): two wavefronts; (16, 40): h = 20 over 16 row groups, two passes, the second ragged; (17, 34): the e / e + LPR
#   boundary of a 16-lane row; (65, 130): 32 lanes; (96, 192): the largest (ndim, 2 ndim) the LDS admits, six passes.
#   "Reject" in a box so small that the objective is nearly flat over it: the walkers stay spread and many proposals leave.
SHAPES = [
    ("sphere", 1, 4, 3, None, None, 5.12),
    ("rastrigin", 1, 6, 4, None, "shared", 5.12),
    ("rosenbrock", 2, 6, 7, None, "per-ensemble", 5.12),
    ("rastrigin", 8, 16, 5, "Reject", None, 0.05),
    ("sphere", 16, 40, 3, None, "per-ensemble", 5.12),
    ("rosenbrock", 17, 34, 2, "Reject", "shared", 0.1),
    ("rastrigin", 65, 130, 2, None, None, 5.12),
    ("sphere", 96, 192, 2, None, None, 5.12),
]
MOVES = {"de": "de", "snooker": "snooker", "four": FOUR}
CASES = [(s, m) for s in SHAPES for m in MOVES if s[2] >= 6 or m == "de"]


@pytest.mark.parametrize("shape,moves", CASES, ids=[f"{s[0]}-n{s[1]}-W{s[2]}-C{s[3]}-{m}" for s, m in CASES])
def test_parity_with_the_restatement_at_every_sample(sa, shape, moves):
    objective, ndim, W, Cn, constraints, x0, half = shape
    bounds = [[-half, half]] * ndim
    span = 2.0 * half
    rs = np.random.RandomState(ndim + W)
    lim = min(2.0, half)
    start = {None: None, "shared": rs.uniform(-lim, lim, (W, ndim)), "per-ensemble": rs.uniform(-lim, lim, (Cn, W, ndim))}[x0]
    base = {"maxiter": 30, "walkers": W, "constraints": constraints, "chains": Cn, "seed": 900 + ndim, "moves": MOVES[moves]}
    seed, want30 = cases.admitted(objective, bounds, start, base)
    for m in (1, 2, 30):
        o = dict(base, maxiter=m, seed=seed)
        print(f"  maxiter {m} seed {seed}")
        with np.errstate(all="ignore"):
            want = want30 if m == 30 else oracle.sample(objective, bounds, x0=start, options=dict(o))
        got = run(sa, getattr(sa.factory, objective), bounds, x0=start, **o)
        check_against(got, want, Cn, W, m, ndim, span, constraints == "Reject")
    total = Cn * W * 29
    assert 0 < want30.nacc.sum() < total  # both outcomes of the decision
    if moves == "four":
        assert set(np.unique(want30.kinds[:, 1:])) == {0, 1, 2, 3}  # every entry within the 30 samples
    if constraints == "Reject":
        assert want30.nfeas.sum() < total  # proposals leave the box
        assert np.all(np.abs(got.xall) <= half)


@pytest.mark.parametrize("external", [False, True], ids=["resident", "batched"])
def test_burn_and_thin_record_rows_of_the_same_run(sa, external):
    """(7, 3): 8 rows; burn = maxiter - 1: one row; thin > maxiter - burn: one row -- rows of the run that records everything, bit
    for bit, the counts and the best values over all samples; with a callback likewise."""
    ndim, W, Cn, m = 5, 12, 4, 30
    bounds = [[-5.12, 5.12]] * ndim
    base = {"maxiter": m, "walkers": W, "chains": Cn, "seed": 31, "moves": FOUR}
    seed, want = cases.admitted("rastrigin", bounds, None, base)
    base["seed"] = seed
    fun = device_objective(sa, "rastrigin") if external else sa.factory.rastrigin
    full = run(sa, fun, bounds, **base)
    check_against(full, want, Cn, W, m, ndim, 10.24, False)
    for burn, thin, rows in ((7, 3, 8), (m - 1, 1, 1), (5, 26, 1), (0, 2, 15)):
        recorded = np.arange(burn, m, thin)
        seen = []
        cut = run(sa, fun, bounds, burn=burn, thin=thin, **base)
        told = run(sa, fun, bounds, burn=burn, thin=thin, **base,
                   callback=lambda xk, state: seen.append((np.array(xk, copy=True), state.nit, state.xall.shape[1])))
        bare = run(sa, fun, bounds, burn=burn, thin=thin, **dict(base, return_all=False))
        for res in (cut, told):
            assert res.xall.shape == (Cn, rows, W, ndim) and res.funall.shape == (Cn, rows, W) and len(recorded) == rows
            assert np.array_equal(res.xall, full.xall[:, recorded]) and np.array_equal(res.funall, full.funall[:, recorded])
        for res in (cut, told, bare):
            assert (res.burn, res.thin) == (burn, thin) and res.moves == full.moves
            for key in ("x", "fun", "accept_ratio", "accept_ratios"):  # over all samples
                assert np.array_equal(res[key], full[key]), key
        assert "xall" not in bare
        assert [s[1] for s in seen] == list(range(1, m + 1)) and np.array_equal(np.stack([s[0] for s in seen], axis=1), full.xall)
        assert [s[2] for s in seen] == [int(np.sum(recorded < max(i, 1))) for i in range(m)]
        with np.errstate(all="ignore"):
            ref = oracle.sample("rastrigin", bounds, options=dict(base, burn=burn, thin=thin))
        check_against(cut, ref, Cn, W, rows, ndim, 10.24, False)


@pytest.mark.parametrize("objective,ndim,W,Cn,constraints,a", [
    ("rastrigin", 3, 8, 7, None, 2.0), ("sphere", 16, 40, 3, None, 2.5), ("styblinski_tang", 70, 140, 2, None, 2.0),
    ("rosenbrock", 5, 12, 20, "Reject", 1.5), ("sphere", 1, 4, 2, None, 3.0)])
def test_one_stretch_entry_is_the_existing_run(sa, objective, ndim, W, Cn, constraints, a):
    """moves=[("stretch", 1, a)] goes through the *_moves entry points, stretch=a through the ones that were there: every
    output is the same, bit for bit, resident and around a caller's objective; burn / thin alone select its rows."""
    half = 1.0 if constraints else 5.12
    bounds = [[-half, half]] * ndim
    o = {"maxiter": 25, "walkers": W, "chains": Cn, "seed": 40 + ndim, "constraints": constraints}
    keys = ("x", "fun", "accept_ratio", "accept_ratios", "xall", "funall") + (("nreject",) if constraints else ())
    for fun in (getattr(sa.factory, objective), device_objective(sa, objective)):
        old = run(sa, fun, bounds, stretch=a, **o)
        new = run(sa, fun, bounds, moves=[("stretch", 1, a)], **o)
        assert "moves" not in old and new.moves == [("stretch", 1.0, a)] and (new.burn, new.thin) == (0, 1)
        for key in keys:
            assert np.array_equal(new[key], old[key], equal_nan=True), key
        thinned = run(sa, fun, bounds, stretch=a, burn=3, thin=4, **o)
        assert thinned.moves == [("stretch", 1.0, a)] and np.array_equal(thinned.xall, old.xall[:, 3::4] if Cn > 1 else old.xall[3::4])
        assert thinned.fun == old.fun and np.array_equal(thinned.accept_ratios, old.accept_ratios)
    assert 0.0 < old.accept_ratio < 1.0


@pytest.mark.parametrize("ndim,W", [(3, 8), (16, 40), (65, 130)])
def test_an_ensemble_does_not_depend_on_its_neighbours_or_the_launches(sa, ndim, W):
    """Ensemble 2 is ensemble 2 among 3 ensembles or among 50, a run cut into one launch per sample by a callback is the run in
    one launch, and a run repeated is the same run -- all bit for bit; the callback's states are the restatement's."""
    bounds = [[-5.12, 5.12]] * ndim
    m = 20
    o = {"maxiter": m, "walkers": W, "seed": 9, "moves": FOUR}
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
        oracle.sample("rastrigin", bounds, options=dict(o, chains=3),
                      callback=lambda xk, state: told.append((xk, state.nit, state.fun, state.x, state.accept_ratio,
                                                              state.xall.shape)))
    for got, ref in zip(seen, told):
        assert close_samples(got[0], ref[0], 10.24) and got[1] == ref[1] and close_values(got[2], ref[2])
        assert close_samples(got[3], ref[3], 10.24) and got[4] == ref[4] and got[5] == ref[5]
    check_against(few, want, 3, W, m, ndim, 10.24, False)
    assert len(set(np.unique(want.kinds[:, 1:]))) == 4


@pytest.mark.parametrize("objective,ndim,W,Cn,constraints,return_all,moves", [
    ("rastrigin", 3, 8, 7, None, True, "four"), ("sphere", 16, 40, 3, None, True, "snooker"),
    ("styblinski_tang", 70, 140, 2, None, True, "four"), ("rosenbrock", 5, 12, 20, "Reject", False, "four"),
    ("sphere", 1, 4, 5, None, True, "de")])
def test_a_callers_objective_gives_the_resident_run(sa, objective, ndim, W, Cn, constraints, return_all, moves):
    """factory.batched of a function that returns sx_eval's values: propose -> fun -> decide per half-sweep is the resident run,
    bit for bit ((16, 40): the resident run walks each half in two passes)."""
    half = 1.0 if constraints else 5.12
    bounds = [[-half, half]] * ndim
    o = {"maxiter": 25, "walkers": W, "chains": Cn, "seed": 40 + ndim, "constraints": constraints, "return_all": return_all,
         "moves": MOVES[moves]}
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


def test_a_torch_objective_beyond_the_lds_limit_agrees_with_the_restatement(sa):
    """ndim 129: rows of 64 lanes, W = 258 -- no resident form; the walkers live in device memory."""
    import torch

    ndim, W, Cn, m = 129, 258, 2, 12
    bounds = [[-5.12, 5.12]] * ndim
    centre = np.linspace(-1.0, 1.0, ndim)
    base = {"maxiter": m, "walkers": W, "chains": Cn, "seed": 66, "moves": FOUR}
    seed, want = cases.admitted(lambda X: (0.7 * (X - centre) ** 2).sum(axis=1), bounds, None, base)
    fun = sa.factory.batched(lambda X, c, s: (s * (X - c) ** 2).sum(dim=1))
    got = run(sa, fun, bounds, args=(torch.tensor(centre, device="cuda"), 0.7), **dict(base, seed=seed))
    check_against(got, want, Cn, W, m, ndim, 10.24, False)
    assert 0 < want.nacc.sum() < Cn * W * (m - 1) and len(set(np.unique(want.kinds[:, 1:]))) >= 3
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
    o = {"maxiter": m, "walkers": W, "chains": Cn, "seed": 3, "moves": FOUR}
    with np.errstate(all="ignore"):
        want = oracle.sample(planted_np, bounds, options=dict(o))
    got = run(sa, sa.factory.batched(planted), bounds, **o)
    f = want.funall
    print("samples: NaN", int(np.isnan(f).sum()), "inf", int(np.isinf(f).sum()), "ties with the previous sample",
          int((f[:, 1:] == f[:, :-1]).sum()))
    assert np.isnan(f).any() and np.isinf(f).any() and np.isfinite(f).any()
    assert np.array_equal(np.isnan(got.funall), np.isnan(f)) and np.array_equal(np.isinf(got.funall), np.isinf(f))
    check_against(got, want, Cn, W, m, 2, 10.24, False)


def test_the_de_move_finds_the_weights_of_two_modes_on_the_device(sa):
    """tests/test_sample_ensemble_moves_host.py's bimodal target through factory.batched, 64 ensembles of 16 walkers, 2 000
    samples of which burn=1000 drops the first half: the share in the heavy mode stays within the host test's bound of 0.75 (the
    yardstick is the mixture, not the device), and the stretch move alone misses it by more than 0.15."""
    import torch

    def bimodal(X):
        rest = (X[:, 1:] ** 2).sum(dim=1)
        qp = ((X[:, 0] - 2.0) ** 2 + rest) / (2.0 * 0.25 ** 2)
        qm = ((X[:, 0] + 2.0) ** 2 + rest) / (2.0 * 0.25 ** 2)
        return -torch.logaddexp(float(np.log(0.75)) - qp, float(np.log(0.25)) - qm)

    fun = sa.factory.batched(bimodal)
    got = run(sa, fun, cases.BIMODAL_BOUNDS, burn=cases.BIMODAL_MAXITER // 2, **cases.bimodal_options("de", 2024))
    assert got.xall.shape == (cases.ENSEMBLES, cases.BIMODAL_MAXITER // 2, cases.WALKERS, cases.BIMODAL_NDIM)
    heavy = got.xall[..., 0] > 0.0
    share, each = float(heavy.mean()), heavy.mean(axis=(1, 2))
    print("share", share, "per ensemble", each.min(), "..", each.max(), "accept_ratio", got.accept_ratio, "bound",
          cases.BIMODAL_BOUND["de"])
    assert abs(share - cases.BIMODAL_SHARE) <= cases.BIMODAL_BOUND["de"]
    o = cases.bimodal_options(None, 2024)
    stretch = run(sa, fun, cases.BIMODAL_BOUNDS, **dict(o, maxiter=500))  # (frozen from the first samples on)
    frozen = float((stretch.xall[:, 250:, :, 0] > 0.0).mean())
    print("stretch alone: share", frozen)
    assert abs(frozen - cases.BIMODAL_SHARE) > cases.STRETCH_MISSES_BY


def test_the_result_object(sa):
    bounds = [[-5.12, 5.12]] * 3
    o = {"maxiter": 30, "seed": 4, "moves": cases.MIXTURE}
    want = oracle.sample("sphere", bounds, options=dict(o, chains=6))
    many = run(sa, sa.factory.sphere, bounds, chains=6, **o)
    one = run(sa, sa.factory.sphere, bounds, chains=1, burn=10, thin=5, **o)
    direct = sa.sample.ensemble(sa.factory.sphere, bounds, chains=6, **o)
    plain = run(sa, sa.factory.sphere, bounds, chains=6, maxiter=30, seed=4)
    assert many.moves == want.moves and np.allclose([e[1] for e in many.moves], [0.7, 0.1, 0.2], rtol=1e-15, atol=0)
    assert [e[0] for e in many.moves] == ["de", "de", "snooker"] and [e[2] for e in many.moves] == [2.38 / np.sqrt(6.0), 1.0, 1.7]
    assert (many.burn, many.thin, many.walkers, many.stretch) == (0, 1, 6, 2.0)
    assert many.xall.shape == (6, 30, 6, 3) and one.xall.shape == (4, 6, 3) and one.funall.shape == (4, 6)
    assert (one.burn, one.thin) == (10, 5) and np.array_equal(one.xall, many.xall[0, 10::5])
    assert np.array_equal(direct.xall, many.xall)
    assert "moves" not in plain and "burn" not in plain and "thin" not in plain
    assert not np.array_equal(plain.xall, many.xall)
    assert many.accept_ratio == want.accept_ratio == want.nacc.sum() / (6 * 6 * 30)
    assert close_values(many.fun, want.fun) and close_samples(many.x, want.x, 10.24)
