"""GPU: tempered sequential Monte Carlo (method="smc"; csrc/sx_sample_smc.hip: the stage kernel, one workgroup per population;
the gather kernel; the mutation kernel, one row group per particle; around a caller's objective a propose and a decide kernel per
step) against the numpy restatement (tests/_smc_oracle.py) stage by stage through the C ABI and through the public call, on
planted values, at its limits, against itself, and on the two targets whose evidence is known.  Tolerances: 1e-6 of the search
range for samples, 1e-6 relative for values, betas, log_evidence, scales and ess; ancestors and acceptance counts are exact.  Seeds
are admitted by the restatement alone (_smc_cases.admitted)."""
import ctypes as C
import os
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _smc_cases as cases  # noqa: E402
import _smc_oracle as oracle  # noqa: E402
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


def run(sa, fun, bounds, callback=None, **options):
    return sa.sample.sample(fun, bounds, method="smc", callback=callback, options=dict(options, rng="philox", backend="hip"))


def check_result(got, want, span):
    """The public call's result against the restated run."""
    assert got.nit == want.nit and got.status == want.status and got.particles == want.particles and got.nfev == want.nfev
    assert np.array_equal(got.stages, want.stages) and np.array_equal(got.statuses, want.statuses)
    for name in ("xall", "funall", "log_evidence", "betas", "accept_ratios", "scales", "ess"):
        assert np.shape(got[name]) == np.shape(want[name]), name
    assert np.array_equal(got.accept_ratios, want.accept_ratios)  # accepted / (P M): the counts, exactly
    assert got.accept_ratio == want.accept_ratio
    assert close_samples(got.xall, want.xall, span) and close_values(got.funall, want.funall)
    assert close_samples(got.x, want.x, span) and close_values(got.fun, want.fun)
    for name in ("betas", "log_evidence", "scales", "ess"):
        assert close_values(got[name], want[name]), name


# ---- 5. parity with the restatement ------------------------------------------------------------------------------------------
def abi_run(sa, fun, bounds, opts, want):
    """The run through the C ABI, one entry point at a time, compared with the restated run's records after every stage."""
    import torch

    from stochopy_amd import _device, _lib, _rng
    from stochopy_amd.sample import _smc

    lower, upper = (np.ascontiguousarray(v, dtype=np.float64) for v in np.transpose(bounds))
    n, Cn, P, M = len(lower), opts["chains"], opts["particles"], opts["steps"]
    s = types.SimpleNamespace(chains=Cn, particles=P, ndim=n, lower=lower, upper=upper, fun_id=_lib.FUN_IDS[fun], steps=M,
                              maxiter=opts["maxiter"], ess=0.5, target=0.234, scale=2.38 / np.sqrt(n),
                              key=_rng.philox_key(opts["seed"]))
    L = _lib.lib()
    ctx = _device.Context()
    span = float(upper[0] - lower[0])
    with torch.cuda.stream(ctx.stream):
        dev, a = _smc.smc_args(ctx, s)

        def call(name, *args):
            _lib.check(getattr(L, name)(C.byref(a), *args, ctx.stream_ptr), name)

        def host(name):
            return dev[name].cpu().numpy()

        call("sx_smc_init")
        for stage in range(1, want.nit + 1):
            took = want.took[stage - 1]
            call("sx_smc_stage", stage)
            anc = host("anc").reshape(Cn, P)
            assert np.array_equal(anc[took], want.ancs[stage - 1][took]), stage  # (a frozen population's are left alone)
            call("sx_smc_resample", stage)
            assert close_values(host("step")[took], want.steps_[stage - 1][took]), stage
            call("sx_smc_mutate", stage)
            assert np.array_equal(host("nacc").reshape(Cn, P)[took], want.naccs[stage - 1][took]), stage
            rec = host("state")
            assert np.array_equal(rec[took, _smc.ST_STAGES], np.full(int(took.sum()), float(stage)))
            assert close_values(rec[:, _smc.ST_BETA], np.atleast_2d(want.betas)[:, stage])
        call("sx_smc_stage", want.nit + 1)  # step 6 of the last stage
        rec = host("state")
        last = np.atleast_1d(want.stages) == want.nit
        assert np.array_equal(rec[last, _smc.ST_COUNT], np.atleast_2d(want.counts)[last, -1].astype(np.float64))
        assert np.array_equal(rec[:, _smc.ST_STATUS], np.atleast_1d(want.statuses).astype(np.float64))
        assert close_values(rec[:, _smc.ST_LOGZ], np.atleast_1d(want.log_evidence))
        x = np.where((np.atleast_1d(want.stages) % 2 == 1).repeat(P)[:, None], host("x1"), host("x0"))
        assert close_samples(x.reshape(Cn, P, n), np.reshape(want.xall, (Cn, P, n)), span)
        ctx.sync()


@pytest.mark.parametrize("case", cases.PARITY, ids=cases.parity_id)
def test_every_stage_is_the_restated_stage(sa, case):
    fun, bounds, opts = cases.parity_setup(case)
    seed, want = cases.admitted(case)
    opts = dict(opts, seed=seed)
    abi_run(sa, fun, bounds, opts, want)
    got = run(sa, getattr(sa.factory, fun), bounds, **opts)
    check_result(got, want, 2.0 * cases.PARITY_BOUND)


# ---- 3. exact cases on planted values ----------------------------------------------------------------------------------------
def device_planted(sa, values):
    import torch

    holder = {}

    def fun(X):
        assert X.shape[0] == len(values)
        if "v" not in holder:
            holder["v"] = torch.from_numpy(np.asarray(values, dtype=np.float64)).to(X.device)
        return holder["v"].clone()

    fun.__name__ = "planted"
    return sa.factory.batched(fun)


def test_constant_values_take_one_stage(sa):
    seen = []
    got = run(sa, device_planted(sa, cases.plant_constant()), cases.PLANT_BOUNDS, particles=cases.PLANT_P, seed=3,
              callback=lambda xk, state: seen.append(state.nit))
    assert got.nit == 1 and got.status == 0 and np.array_equal(got.betas, [0.0, 1.0]) and got.log_evidence == -2.5
    assert got.ess[0] == 1.0 and seen == [1]
    want = oracle.sample(cases.planted(cases.plant_constant()), cases.PLANT_BOUNDS, {"particles": cases.PLANT_P, "seed": 3})
    check_result(got, want, 3.0)  # (the ancestors were the identity: particle i is the restatement's particle i, moved alike)


def test_one_finite_value_is_every_ancestor_and_the_floor_keeps_the_run_going(sa):
    values = cases.plant_one_finite()
    first = []
    got = run(sa, device_planted(sa, values), cases.PLANT_BOUNDS, particles=cases.PLANT_P, seed=3, maxiter=3,
              callback=lambda xk, state: first.append(xk.copy()))
    want = oracle.sample(cases.planted(values), cases.PLANT_BOUNDS, {"particles": cases.PLANT_P, "seed": 3, "maxiter": 3},
                         record=True)
    assert np.all(want.ancs[0] == 37) and got.nit == want.nit >= 2
    assert np.ptp(first[0], axis=0).max() <= 1e-6  # one point, moved by the floor's steps: 1e-8 of the half-width
    assert got.betas[1] == 2.0 ** -52
    check_result(got, want, 3.0)


@pytest.mark.parametrize("middle", ["none", "neginf"])
def test_a_population_without_a_usable_value_ends_alone(sa, middle):
    values = cases.plant_mixed(middle)
    got = run(sa, device_planted(sa, values), cases.PLANT_BOUNDS, particles=cases.PLANT_P, chains=3, seed=3)
    want = oracle.sample(cases.planted(values), cases.PLANT_BOUNDS, {"particles": cases.PLANT_P, "chains": 3, "seed": 3})
    assert list(got.statuses) == [0, -2, 0] and got.status == -2 and got.log_evidence[1] == -np.inf and got.stages[1] == 0
    assert np.all(got.ess[1] == 0.0) and np.all(got.betas[1] == 0.0)
    check_result(got, want, 3.0)


def test_maxiter_one_on_a_hard_target_stops_below_one(sa):
    bounds = [[-5.12, 5.12]] * 40
    got = run(sa, sa.factory.rosenbrock, bounds, particles=64, chains=2, seed=5, maxiter=1)
    assert list(got.statuses) == [-1, -1] and got.status == -1 and got.nit == 1 and np.all(got.betas[:, -1] < 1.0)
    assert np.all(got.betas[:, -1] > 0.0) and got.betas.shape == (2, 2)
    want = oracle.sample("rosenbrock", bounds, {"particles": 64, "chains": 2, "seed": 5, "maxiter": 1})
    assert np.array_equal(got.accept_ratios, want.accept_ratios) and close_values(got.betas, want.betas)


# ---- 6. limits --------------------------------------------------------------------------------------------------------------
def test_the_most_particles_of_a_population(sa):
    from stochopy_amd import _lib

    P = int(_lib.lib().sx_smc_max_particles())
    bounds = [[-5.12, 5.12]] * 2
    got = run(sa, sa.factory.sphere, bounds, particles=P, seed=2, steps=2)
    want = oracle.sample("sphere", bounds, {"particles": P, "seed": 2, "steps": 2})
    print("    stages", got.nit, "log_evidence", got.log_evidence, want.log_evidence)
    assert got.nit == want.nit and got.status == 0 and got.xall.shape == (P, 2)
    assert close_values(got.betas, want.betas) and close_values(got.log_evidence, want.log_evidence)
    assert abs(got.log_evidence - 2.0 * np.log(np.sqrt(np.pi) / 10.24)) < 0.1  # (the exact value up to erf(5.12) = 1 - 4e-13)
    with pytest.raises(ValueError, match="particles"):
        run(sa, sa.factory.sphere, bounds, particles=P + 1, seed=2)


def test_the_longest_row(sa):
    from stochopy_amd import _lib

    n = _lib.wide_from()
    got = run(sa, sa.factory.sphere, [[-5.12, 5.12]] * n, particles=8, seed=2, steps=2, maxiter=2)
    want = oracle.sample("sphere", [[-5.12, 5.12]] * n, {"particles": 8, "seed": 2, "steps": 2, "maxiter": 2})
    assert got.xall.shape == (8, n) and got.nit == want.nit
    assert np.array_equal(got.accept_ratios, want.accept_ratios) and close_values(got.betas, want.betas)
    assert close_values(got.log_evidence, want.log_evidence)
    with pytest.raises(ValueError, match=str(n)):
        run(sa, sa.factory.sphere, [[-5.12, 5.12]] * (n + 1), particles=8, seed=2)


# ---- 7. invariances ---------------------------------------------------------------------------------------------------------
KEYS = ("x", "fun", "xall", "funall", "log_evidence", "betas", "stages", "statuses", "accept_ratios", "scales", "ess")
ROSEN = {"particles": 100, "steps": 4, "seed": 9}
ROSEN_BOUNDS = [[-2.0, 2.0]] * 5


@pytest.fixture(scope="module")
def rosen3(sa):
    return run(sa, sa.factory.rosenbrock, ROSEN_BOUNDS, chains=3, **ROSEN)


def test_a_run_repeats_itself(sa, rosen3):
    again = run(sa, sa.factory.rosenbrock, ROSEN_BOUNDS, chains=3, **ROSEN)
    assert rosen3.nit >= 3 and rosen3.status == 0
    for key in KEYS:
        assert np.array_equal(rosen3[key], again[key]), key


def test_a_population_does_not_depend_on_the_others(sa, rosen3):
    many = run(sa, sa.factory.rosenbrock, ROSEN_BOUNDS, chains=50, **ROSEN)
    S = int(rosen3.stages[2])
    assert many.stages[2] == S
    for key in ("xall", "funall", "log_evidence", "statuses"):
        assert np.array_equal(rosen3[key][2], many[key][2]), key
    for key in ("betas", "accept_ratios", "scales", "ess"):
        assert np.array_equal(rosen3[key][2][:S], many[key][2][:S]), key


def test_a_callers_objective_with_the_kernels_values_is_the_resident_run(sa, rosen3):
    got = run(sa, device_objective(sa, "rosenbrock"), ROSEN_BOUNDS, chains=3, **ROSEN)
    for key in KEYS:
        assert np.array_equal(rosen3[key], got[key]), key
    assert got.nfev == rosen3.nfev and got.accept_ratio == rosen3.accept_ratio


def test_a_callback_sees_every_stage_and_changes_nothing(sa, rosen3):
    seen = []
    got = run(sa, sa.factory.rosenbrock, ROSEN_BOUNDS, chains=3, callback=lambda xk, state: seen.append((xk.copy(), dict(state))),
              **ROSEN)
    for key in KEYS:
        assert np.array_equal(rosen3[key], got[key]), key
    assert [state["nit"] for _, state in seen] == list(range(1, got.nit + 1))
    assert all(xk.shape == (3, 100, 5) for xk, _ in seen) and np.array_equal(seen[-1][0], got.xall)
    assert np.array_equal(seen[-1][1]["betas"], got.betas) and np.array_equal(seen[-1][1]["log_evidence"], got.log_evidence)
    assert seen[0][1]["betas"].shape == (3, 2)


# ---- 8. the statistics on the device -----------------------------------------------------------------------------------------
def device_bimodal(sa):
    import torch

    def fun(X):
        rest = (X[:, 1:] ** 2).sum(dim=1)
        qp = ((X[:, 0] - 2.0) ** 2 + rest) / (2.0 * 0.25 ** 2)
        qm = ((X[:, 0] + 2.0) ** 2 + rest) / (2.0 * 0.25 ** 2)
        return -torch.logaddexp(np.log(0.75) - qp, np.log(0.25) - qm)

    fun.__name__ = "bimodal"
    return sa.factory.batched(fun)


def test_the_sphere_has_its_evidence_and_its_variance(sa):
    got = run(sa, sa.factory.sphere, cases.SPHERE_BOUNDS, seed=cases.GPU_SEED, **cases.SPHERE_OPTIONS)
    dz, dv = cases.sphere_statistics(got)
    print("    stages", got.nit, "|dlogZ|", dz, "bound", cases.BOUND["sphere_logz"], "|dvar|", dv, "bound", cases.BOUND["sphere_variance"])
    assert got.status == 0 and dz <= cases.BOUND["sphere_logz"] and dv <= cases.BOUND["sphere_variance"]


def test_the_bimodal_target_has_its_evidence_and_its_mode_weights(sa):
    got = run(sa, device_bimodal(sa), cases.BIMODAL_BOUNDS, seed=cases.GPU_SEED, **cases.BIMODAL_OPTIONS)
    dz, ds = cases.bimodal_statistics(got)
    print("    stages", got.nit, "|dlogZ|", dz, "bound", cases.BOUND["bimodal_logz"], "|dshare|", ds, "bound", cases.BOUND["bimodal_share"])
    assert got.status == 0 and dz <= cases.BOUND["bimodal_logz"] and ds <= cases.BOUND["bimodal_share"]
