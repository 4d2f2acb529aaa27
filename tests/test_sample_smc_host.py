"""No GPU: tempered sequential Monte Carlo of stochopy_amd.sample (method="smc") -- the options' validation (every refusal is
raised before the device is touched), the dispatch, the C ABI additions, and the numpy restatement (tests/_smc_oracle.py): its
evidence, variance and mode weights on the two targets of tests/_smc_cases.py, where the restated mcmc chains miss the mode
weights; its exact cases on planted values; its determinism."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _smc_cases as cases  # noqa: E402
import _smc_oracle as oracle  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sa():
    import stochopy_amd

    return stochopy_amd


@pytest.fixture()
def no_device(monkeypatch):
    """Any attempt to open the device fails the test."""
    from stochopy_amd import _device

    def refuse(*a, **k):
        raise AssertionError("the device was touched")

    monkeypatch.setattr(_device, "Context", refuse)


def call(sa, ndim=4, fun=None, x0=None, args=(), callback=None, **options):
    o = dict({"chains": 2, "seed": 1}, **options)
    return sa.sample.sample(sa.factory.sphere if fun is None else fun, [[-5.12, 5.12]] * ndim, x0=x0, args=args, method="smc",
                            options=o, callback=callback)


# ---- 1. refusals and accepted forms -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("options,error,names", [
    ({"particles": 3}, ValueError, "particles"),
    ({"particles": 0}, ValueError, "particles"),
    ({"particles": 16385}, ValueError, "particles"),
    ({"particles": True}, TypeError, "particles"),
    ({"particles": 64.0}, TypeError, "particles"),
    ({"particles": "64"}, TypeError, "particles"),
    ({"chains": 0}, ValueError, "chains"),
    ({"chains": True}, ValueError, "chains"),
    ({"chains": 1.5}, ValueError, "chains"),
    ({"steps": 0}, ValueError, "steps"),
    ({"steps": -1}, ValueError, "steps"),
    ({"steps": True}, TypeError, "steps"),
    ({"steps": 2.0}, TypeError, "steps"),
    ({"ess": 0.0}, ValueError, "ess"),
    ({"ess": 1.0}, ValueError, "ess"),
    ({"ess": np.nan}, ValueError, "ess"),
    ({"ess": "0.5"}, TypeError, "ess"),
    ({"ess": True}, TypeError, "ess"),
    ({"target_accept": 0.0}, ValueError, "target_accept"),
    ({"target_accept": 1.0}, ValueError, "target_accept"),
    ({"target_accept": -0.2}, ValueError, "target_accept"),
    ({"target_accept": None}, TypeError, "target_accept"),
    ({"target_accept": False}, TypeError, "target_accept"),
    ({"scale": 0.0}, ValueError, "scale"),
    ({"scale": -1.0}, ValueError, "scale"),
    ({"scale": np.inf}, ValueError, "scale"),
    ({"scale": np.nan}, ValueError, "scale"),
    ({"scale": "1"}, TypeError, "scale"),
    ({"scale": True}, TypeError, "scale"),
    ({"maxiter": 0}, ValueError, "maxiter"),
    ({"maxiter": True}, ValueError, "maxiter"),
    ({"maxiter": 1 << 28, "steps": 8}, ValueError, "maxiter"),   # maxiter * steps = 2^31
    ({"seed": None}, ValueError, "seed"),
    ({"seed": True}, ValueError, "seed"),
    ({"seed": 1.0}, ValueError, "seed"),
    ({"rng": "numpy-legacy"}, ValueError, "rng"),
    ({"rng": "numpy-legacy", "chains": 1}, ValueError, "rng"),
    ({"rng": "mt"}, ValueError, "rng"),
    ({"backend": "cuda"}, ValueError, "backend"),
    ({"x0": np.zeros(4)}, ValueError, "x0"),
    ({"x0": np.zeros((2, 1024, 4))}, ValueError, "x0"),
    ({"args": (1.0,)}, TypeError, "args"),
])
def test_refusals_name_the_option_and_come_before_the_device(sa, no_device, options, error, names):
    with pytest.raises(error, match=names):
        call(sa, **options)


def test_other_refusals_come_before_the_device(sa, no_device):
    with pytest.raises(TypeError, match="plain Python callables"):
        call(sa, fun=lambda x: float(np.sum(x * x)))
    with pytest.raises(TypeError):
        call(sa, fun=3)
    with pytest.raises(ValueError):  # the reference's bare errors: bounds, callback -- before this backend's own
        sa.sample.sample(sa.factory.sphere, [-5.0, 5.0], method="smc", options={"seed": 1, "particles": 3})
    with pytest.raises(ValueError) as e:
        sa.sample.sample(sa.factory.sphere, [[-5.0, 5.0]] * 4, method="smc", callback=3, options={"seed": 1, "particles": 3})
    assert str(e.value) == ""
    with pytest.raises(TypeError):  # constraints, warmup, burn, thin, temperatures are no options of this method
        call(sa, constraints="Reject")
    with pytest.raises(TypeError):
        call(sa, warmup=10)
    from stochopy_amd import _lib
    with pytest.raises(ValueError, match=str(_lib.wide_from())):
        call(sa, ndim=_lib.wide_from() + 1)
    with pytest.raises(ValueError, match="particles"):
        call(sa, particles=int(_lib.lib().sx_smc_max_particles()) + 1)


@pytest.mark.parametrize("options", [
    {}, {"particles": 4}, {"particles": 16384}, {"particles": np.int64(100)}, {"chains": 1}, {"steps": 1}, {"steps": np.int32(3)},
    {"ess": 0.9}, {"ess": np.float32(0.25)}, {"target_accept": 0.5}, {"scale": 1}, {"scale": np.float64(0.3)}, {"scale": None},
    {"maxiter": 1}, {"maxiter": (1 << 28) - 1, "steps": 8}, {"seed": np.int64(3)}, {"seed": -5}, {"rng": "philox"},
    {"backend": "hip"}, {"callback": lambda xk, state: None}, {"ndim": 1}, {"ndim": 2048, "particles": 8}])
def test_accepted_values_reach_the_device(sa, no_device, options):
    with pytest.raises(AssertionError, match="the device was touched"):
        call(sa, **options)


def test_a_callers_objective_and_its_args_reach_the_device(sa, no_device):
    fun = sa.factory.batched(lambda X, a: a * (X * X).sum(dim=1))
    with pytest.raises(AssertionError, match="the device was touched"):
        call(sa, fun=fun, args=(2.0,))


def test_dispatch(sa, monkeypatch):
    from stochopy_amd.sample import _helpers, _smc

    assert set(_helpers._sampler_map) == {"mcmc", "hmc"}
    assert _helpers._own_sampler_map["smc"] is sa.sample.smc is _smc.sample
    assert "smc" in sa.sample.__all__ and 'method="smc"' in _helpers.sample.__doc__
    monkeypatch.setattr(_smc, "run", lambda s: s)
    s = call(sa)
    assert (s.particles, s.chains, s.steps, s.ess, s.target, s.maxiter) == (1024, 2, 8, 0.5, 0.234, 100)
    assert s.scale == 2.38 / np.sqrt(4) and s.external is None and s.x0 is None
    s = call(sa, ndim=9, particles=64, steps=3, ess=0.7, target_accept=0.3, scale=0.5, maxiter=7, chains=5)
    assert (s.particles, s.chains, s.steps, s.ess, s.target, s.scale, s.maxiter, s.ndim) == (64, 5, 3, 0.7, 0.3, 0.5, 7, 9)
    for word in ("HMC", "x0", "adaptive ``steps``", "Weighted output".lower(), "workgroup's LDS", "numpy-legacy", "several GPUs"):
        assert word in _smc.sample.__doc__, word


def test_abi(sa):
    """Declared in the header, exported, bound, with the argument types of the declaration; the struct's mirror has its size."""
    from stochopy_amd import _lib

    header = open(os.path.join(ROOT, "include", "stochopy_hip.h")).read()
    lib = _lib.lib()
    vp = C.c_void_p
    args = C.POINTER(_lib.SxSmcArgs)
    want = {
        "sx_smc_args_bytes": [],
        "sx_smc_max_particles": [],
        "sx_smc_init": [args, vp],
        "sx_smc_stage": [args, C.c_int, vp],
        "sx_smc_resample": [args, C.c_int, vp],
        "sx_smc_mutate": [args, C.c_int, vp],
        "sx_smc_propose": [args, C.c_int, C.c_int, vp, vp],
        "sx_smc_decide": [args, C.c_int, C.c_int, vp, vp, vp],
    }
    ctype = {"const sx_smc_args *": args, "int": C.c_int, "void *": vp, "double *": vp, "const double *": vp}
    for name, argtypes in want.items():
        assert _lib.PROTOTYPES[name] == (C.c_int, argtypes)
        assert getattr(lib, name).argtypes == argtypes and getattr(lib, name).restype is C.c_int
        decl = re.search(r"^int " + name + r"\(([^)]*)\)", header, re.M).group(1)
        declared = [] if decl.strip() == "void" else \
            [re.match(r"(.*?)(\w+)$", " ".join(p.split())).group(1).strip() for p in decl.split(",")]
        assert [ctype[d] for d in declared] == argtypes, (name, declared)
    assert lib.sx_smc_args_bytes() == C.sizeof(_lib.SxSmcArgs) and lib.sx_struct_size(13) <= 0
    assert lib.sx_smc_max_particles() == oracle.MAX_PARTICLES == 16384 and 8 * 16384 + 1024 <= 160 * 1024
    device = open(os.path.join(ROOT, "stochopy_amd", "csrc", "sx_device.hpp")).read()
    assert "kPurposeSampleResample = 18" in device and oracle.PURPOSE_RESAMPLE == 18
    assert "Tempered sequential Monte Carlo" in header


def test_the_entry_points_check_their_arguments(sa):
    """-1 and a message, as check_sample_args does, before anything is launched (no device is needed to be refused)."""
    from stochopy_amd import _lib

    L = _lib.lib()
    one = C.c_void_p(8)  # (never followed: every call below is refused)

    def args(**change):
        a = _lib.SxSmcArgs()
        a.x[0] = a.x[1] = a.f[0] = a.f[1] = 8
        a.anc = a.nacc = a.step = a.state = a.lower = a.upper = one
        a.C, a.P, a.n, a.fun_id, a.steps, a.maxiter = 2, 64, 3, 5, 8, 10
        a.ess, a.target, a.scale = 0.5, 0.234, 1.0
        for k, v in change.items():
            setattr(a, k, v)
        return a

    def refused(rc, word):
        assert rc == -1 and word in L.sx_last_error().decode(), L.sx_last_error().decode()

    refused(L.sx_smc_init(None, None), "sx_smc_init: null args")
    refused(L.sx_smc_init(C.byref(args(state=None)), None), "null state pointer")
    refused(L.sx_smc_init(C.byref(args(upper=None)), None), "bounds")
    refused(L.sx_smc_init(C.byref(args(P=3)), None), "bad shape")
    refused(L.sx_smc_init(C.byref(args(P=16385)), None), "bad shape")
    refused(L.sx_smc_init(C.byref(args(C=0)), None), "bad shape")
    refused(L.sx_smc_init(C.byref(args(C=1 << 20, P=4096)), None), "bad shape")
    refused(L.sx_smc_init(C.byref(args(n=0)), None), "rows of")
    refused(L.sx_smc_init(C.byref(args(n=_lib.wide_from() + 1)), None), "rows of")
    refused(L.sx_smc_init(C.byref(args(fun_id=7)), None), "unknown objective")
    refused(L.sx_smc_mutate(C.byref(args(fun_id=-1)), 1, None), "sx_smc_mutate: unknown objective")
    refused(L.sx_smc_stage(C.byref(args(steps=0)), 1, None), "steps")
    refused(L.sx_smc_stage(C.byref(args(maxiter=1 << 28)), 1, None), "steps")
    refused(L.sx_smc_stage(C.byref(args(ess=1.0)), 1, None), "ess")
    refused(L.sx_smc_stage(C.byref(args(target=0.0)), 1, None), "target")
    refused(L.sx_smc_stage(C.byref(args(scale=float("inf"))), 1, None), "scale")
    refused(L.sx_smc_stage(C.byref(args()), 0, None), "sx_smc_stage: stage")
    refused(L.sx_smc_stage(C.byref(args()), 12, None), "stage")       # maxiter + 1 = 11 is the closing call
    refused(L.sx_smc_resample(C.byref(args()), 11, None), "sx_smc_resample: stage")
    refused(L.sx_smc_resample(C.byref(args()), 0, None), "stage")
    refused(L.sx_smc_mutate(C.byref(args()), 0, None), "stage")
    refused(L.sx_smc_mutate(C.byref(args()), -1, None), "stage")
    refused(L.sx_smc_propose(C.byref(args()), 1, 1, None, None), "sx_smc_propose: null proposal")
    refused(L.sx_smc_propose(C.byref(args()), 1, 0, one, None), "step outside")
    refused(L.sx_smc_propose(C.byref(args()), 1, 9, one, None), "step outside")
    refused(L.sx_smc_propose(C.byref(args()), 0, 1, one, None), "step outside")
    refused(L.sx_smc_decide(C.byref(args()), 1, 1, one, None, None), "sx_smc_decide: null proposal")
    refused(L.sx_smc_decide(C.byref(args()), 11, 1, one, one, None), "stage")
    refused(L.sx_smc_decide(C.byref(args(fun_id=99)), 1, 9, one, one, None), "step outside")  # (fun_id is not read here)


# ---- 2. the restatement on the two targets -----------------------------------------------------------------------------------
def test_the_bounds_are_within_their_caps():
    assert set(cases.BOUND) == set(cases.CAP)
    for name, bound in cases.BOUND.items():
        assert 0.0 < bound <= cases.CAP[name], name
    recorded = open(os.path.join(ROOT, "profiles", "sample_smc_cases.txt")).read()
    for name, value in cases.LARGEST_DEVIATION.items():
        assert re.search(rf"{name}\s+largest deviation\s+{value:.4f}\b", recorded), name


@pytest.fixture(scope="module")
def restated():
    """The restated runs of the two targets for the tests' seeds: computed once, left unchanged."""
    runs = {}
    for seed in cases.TEST_SEEDS:
        runs["sphere", seed] = oracle.sample("sphere", cases.SPHERE_BOUNDS, dict(cases.SPHERE_OPTIONS, seed=seed))
        runs["bimodal", seed] = oracle.sample(cases.bimodal_value, cases.BIMODAL_BOUNDS, dict(cases.BIMODAL_OPTIONS, seed=seed))
    return runs


@pytest.mark.parametrize("seed", cases.TEST_SEEDS)
def test_the_sphere_has_its_evidence_and_its_variance(restated, seed):
    res = restated["sphere", seed]
    dz, dv = cases.sphere_statistics(res)
    print("    stages", res.nit, "|dlogZ|", dz, "|dvar|", dv)
    assert res.status == 0 and res.nit == 5
    assert dz <= cases.BOUND["sphere_logz"] and dv <= cases.BOUND["sphere_variance"]


@pytest.mark.parametrize("seed", cases.TEST_SEEDS)
def test_the_bimodal_target_has_its_evidence_and_its_mode_weights(restated, seed):
    res = restated["bimodal", seed]
    dz, ds = cases.bimodal_statistics(res)
    print("    stages", res.nit, "|dlogZ|", dz, "|dshare|", ds)
    assert res.status == 0 and res.nit == 7
    assert dz <= cases.BOUND["bimodal_logz"] and ds <= cases.BOUND["bimodal_share"]


def test_plain_chains_miss_the_mode_weights(monkeypatch):
    """The target discriminates: 16 x 1 024 restated mcmc chains from a uniform start, as many evaluations each as a particle of
    the smc run had (1 + 7 stages x 8 steps), stay in the mode they first reach."""
    import _sample_oracle
    from oracle import objectives

    monkeypatch.setitem(objectives.OBJECTIVES, "bimodal", cases.bimodal_value)
    res = _sample_oracle.sample("bimodal", cases.BIMODAL_BOUNDS, method="mcmc",
                                options={"chains": 16 * 1024, "maxiter": 57, "seed": 1, "rng": "philox", "stepsize": 0.1})
    share = float((res.xall[:, -1, 0] > 0.0).mean())
    print("    share of the chains' last samples in the heavy mode", share)
    assert abs(share - cases.BIMODAL_SHARE) > cases.MCMC_MISSES_BY


# ---- 3. exact cases ----------------------------------------------------------------------------------------------------------
def test_constant_values_take_one_stage():
    res = oracle.sample(cases.planted(cases.plant_constant()), cases.PLANT_BOUNDS, {"particles": cases.PLANT_P, "seed": 3},
                        record=True)
    assert res.nit == 1 and res.status == 0 and np.array_equal(res.betas, [0.0, 1.0]) and res.log_evidence == -2.5
    assert np.array_equal(res.ancs[0][0], np.arange(cases.PLANT_P)) and res.ess[0] == 1.0
    assert res.nfev == cases.PLANT_P * (1 + 8)


def test_one_finite_value_is_every_ancestor_and_the_floor_keeps_the_run_going():
    res = oracle.sample(cases.planted(cases.plant_one_finite()), cases.PLANT_BOUNDS,
                        {"particles": cases.PLANT_P, "seed": 3, "maxiter": 3}, record=True)
    assert np.all(res.ancs[0] == 37) and res.nit >= 2 and res.betas[1] == 2.0 ** -52
    floor = 1.0e-8 * 1.5  # the half-width of PLANT_BOUNDS
    assert np.array_equal(res.steps_[0][0], np.full(cases.PLANT_NDIM, (2.38 / np.sqrt(cases.PLANT_NDIM)) * floor))
    assert res.accept_ratios[0] > 0.0 and np.ptp(res.xall, axis=0).max() > 0.0  # it moved


@pytest.mark.parametrize("middle", ["none", "neginf"])
def test_a_population_without_a_usable_value_ends_alone(middle):
    values = cases.plant_mixed(middle)
    res = oracle.sample(cases.planted(values), cases.PLANT_BOUNDS, {"particles": cases.PLANT_P, "chains": 3, "seed": 3})
    assert list(res.statuses) == [0, -2, 0] and res.status == -2 and res.log_evidence[1] == -np.inf and res.stages[1] == 0
    assert np.all(np.isfinite(res.log_evidence[[0, 2]])) and np.all(res.betas[[0, 2], -1] == 1.0)
    # the others are what they are without it
    alone = oracle.sample(cases.planted(cases.plant_mixed("none")), cases.PLANT_BOUNDS, {"particles": cases.PLANT_P, "chains": 3, "seed": 3})
    for key in ("xall", "funall", "log_evidence", "betas"):
        assert np.array_equal(res[key][[0, 2]], alone[key][[0, 2]]), key


def test_every_population_without_a_usable_value():
    values = np.full(2 * cases.PLANT_P, np.inf)
    res = oracle.sample(cases.planted(values), cases.PLANT_BOUNDS, {"particles": cases.PLANT_P, "chains": 2, "seed": 3})
    assert res.nit == 0 and list(res.statuses) == [-2, -2] and res.betas.shape == (2, 1) and res.ess.shape == (2, 0)
    assert res.nfev == 2 * cases.PLANT_P and res.accept_ratio == 0.0


def test_maxiter_one_on_a_hard_target_stops_below_one():
    res = oracle.sample("rosenbrock", [[-5.12, 5.12]] * 40, {"particles": 64, "chains": 2, "seed": 5, "maxiter": 1})
    assert list(res.statuses) == [-1, -1] and res.status == -1 and res.nit == 1 and np.all(res.betas[:, -1] < 1.0)


# ---- 4. determinism of the rule ----------------------------------------------------------------------------------------------
def test_a_population_does_not_depend_on_the_others():
    o = {"particles": 100, "steps": 4, "seed": 9}
    bounds = [[-2.0, 2.0]] * 5
    three = oracle.sample("rosenbrock", bounds, dict(o, chains=3))
    alone = oracle.sample("rosenbrock", bounds, dict(o, chains=1, pop0=2))  # population 2 of any call: keyed by its global rows
    S = int(three.stages[2])
    assert alone.nit == S
    for key in ("xall", "funall", "log_evidence"):
        assert np.array_equal(three[key][2], alone[key]), key
    for key in ("betas", "accept_ratios", "scales", "ess"):
        assert np.array_equal(three[key][2][:len(alone[key])], alone[key]), key
    fifty = oracle.sample("rosenbrock", bounds, dict(o, chains=50))
    for key in ("xall", "funall", "log_evidence"):
        assert np.array_equal(three[key][2], fifty[key][2]), key
    for res in (three, fifty):
        for c in range(len(res.stages)):
            b = res.betas[c][:res.stages[c] + 1]
            assert res.statuses[c] == 0 and b[0] == 0.0 and b[-1] == 1.0 and np.all(np.diff(b) > 0.0)
            assert np.all(res.betas[c][res.stages[c]:] == 1.0)


def test_every_parity_case_admits_a_seed():
    for case in cases.PARITY:
        seed, run = cases.admitted(case)
        assert cases.parity_setup(case)[2]["seed"] <= seed < cases.parity_setup(case)[2]["seed"] + 8
    assert {c[0] for c in cases.PARITY} == {"ackley", "griewank", "quartic", "rastrigin", "rosenbrock", "sphere", "styblinski_tang"}
    assert {c[1] for c in cases.PARITY} == {1, 2, 3, 64, 65, 128, 129, 300} and {c[2] for c in cases.PARITY} == {4, 63, 64, 100, 1025}
    assert {c[3] for c in cases.PARITY} == {1, 3} and 18 <= len(cases.PARITY) <= 24
