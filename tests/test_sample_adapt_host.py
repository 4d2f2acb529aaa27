"""No GPU: per-chain step-size adaptation in a warm-up, burn-in and thinning for stochopy_amd.sample (options warmup /
target_accept / burn / thin) -- the options' validation (every refusal is raised before the device is touched), the C ABI
additions, and the numpy restatement (tests/_sample_adapt_oracle.py): its link to the plain restatement and the
statistical claims the GPU test relies on."""
import ctypes as C
import functools
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _sample_adapt_oracle  # noqa: E402
import _sample_oracle  # noqa: E402

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


def call(sa, method="mcmc", ndim=4, **options):
    o = dict({"rng": "philox", "chains": 2, "maxiter": 5, "seed": 1}, **options)
    return sa.sample.sample(sa.factory.sphere, [[-5.12, 5.12]] * ndim, method=method, options=o)


REFUSALS = [
    # out of range
    ({"warmup": -1}, ValueError, "warmup"),
    ({"warmup": 5}, ValueError, "warmup"),                       # maxiter - 1 = 4 is the most
    ({"warmup": 2, "target_accept": 0.0}, ValueError, "target_accept"),
    ({"warmup": 2, "target_accept": 1.0}, ValueError, "target_accept"),
    ({"warmup": 2, "target_accept": -0.3}, ValueError, "target_accept"),
    ({"warmup": 2, "target_accept": float("nan")}, ValueError, "target_accept"),
    ({"burn": -1}, ValueError, "burn"),
    ({"burn": 5}, ValueError, "burn"),
    ({"thin": 0}, ValueError, "thin"),
    ({"thin": -2}, ValueError, "thin"),
    # target_accept without warmup
    ({"target_accept": 0.3}, ValueError, "target_accept"),
    ({"target_accept": 0.3, "warmup": 0, "burn": 1}, ValueError, "target_accept"),
    # wrong types
    ({"warmup": 2.0}, TypeError, "warmup"),
    ({"warmup": True}, TypeError, "warmup"),
    ({"warmup": "2"}, TypeError, "warmup"),
    ({"warmup": None}, TypeError, "warmup"),
    ({"warmup": 2, "target_accept": "0.3"}, TypeError, "target_accept"),
    ({"warmup": 2, "target_accept": True}, TypeError, "target_accept"),
    ({"burn": 1.0}, TypeError, "burn"),
    ({"burn": False}, TypeError, "burn"),
    ({"thin": 2.0}, TypeError, "thin"),
    ({"thin": True}, TypeError, "thin"),
    ({"thin": None}, TypeError, "thin"),
    # any of the four with rng != "philox"
    ({"warmup": 2, "rng": "numpy-legacy", "chains": 1}, ValueError, "warmup"),
    ({"warmup": 2, "target_accept": 0.3, "rng": "numpy-legacy", "chains": 1}, ValueError, "target_accept"),
    ({"burn": 1, "rng": "numpy-legacy", "chains": 1}, ValueError, "burn"),
    ({"thin": 2, "rng": "numpy-legacy", "chains": 1}, ValueError, "thin"),
]


@pytest.mark.parametrize("method", ["mcmc", "hmc"])
@pytest.mark.parametrize("options,error,name", REFUSALS)
def test_refusals_name_the_option_and_come_before_the_device(sa, no_device, method, options, error, name):
    with pytest.raises(error, match=name):
        call(sa, method=method, **options)


@pytest.mark.parametrize("options,name", [({"warmup": 2}, "warmup"), ({"warmup": 2, "target_accept": 0.3}, "target_accept"),
                                          ({"burn": 1}, "burn"), ({"thin": 2}, "thin")])
def test_refused_with_temperatures(sa, no_device, options, name):
    with pytest.raises(ValueError, match=name):
        call(sa, temperatures=[1.0, 2.0, 4.0], **options)
    with pytest.raises(ValueError, match=name):
        call(sa, temperatures=[1.0, 2.0, 4.0], swap_every=2, **options)
    with pytest.raises(ValueError, match=name):
        call(sa, method="hmc", temperatures=[1.0, 2.0, 4.0], **options)


def test_the_reference_errors_come_first(sa, no_device):
    with pytest.raises(ValueError) as e:  # (bounds that are no (ndim, 2) array: the reference's bare ValueError)
        sa.sample.sample(sa.factory.sphere, [1.0, 2.0], method="mcmc", options={"rng": "philox", "warmup": "x"})
    assert str(e.value) == ""
    with pytest.raises(ValueError) as e:
        call(sa, perc=1.5, warmup="x")
    assert str(e.value) == ""
    with pytest.raises(ValueError) as e:
        call(sa, method="hmc", nleap=0, warmup="x")
    assert str(e.value) == ""


def test_every_accepted_value_passes_the_checks(sa, no_device):
    """(the device is what refuses here: every check passed)"""
    for options in ({"warmup": 4}, {"warmup": np.int64(1)}, {"warmup": 2, "target_accept": 0.5},
                    {"warmup": 1, "target_accept": np.float32(0.25)}, {"burn": 0}, {"burn": 4}, {"thin": 1000},
                    {"warmup": 2, "burn": 0, "thin": 3}):
        for method in ("mcmc", "hmc"):
            with pytest.raises(AssertionError, match="the device was touched"):
                call(sa, method=method, **options)


def test_with_default_options_the_call_path_is_untouched(sa, monkeypatch):
    from stochopy_amd.sample import _chains

    seen = []
    monkeypatch.setattr(_chains, "run", lambda s: seen.append(s) or "plain")
    for method in ("mcmc", "hmc"):
        assert call(sa, method=method) == "plain"
        assert call(sa, method=method, warmup=0, target_accept=None, burn=None, thin=1) == "plain"
    assert len(seen) == 4 and all(s.adapt is None for s in seen)
    # set options arrive checked, with the method's default target and burn = warmup
    call(sa, warmup=3)
    call(sa, warmup=3, perc=0.25)              # k == 1
    call(sa, method="hmc", warmup=3, thin=2)
    call(sa, method="hmc", warmup=2, target_accept=0.8, burn=0)
    call(sa, thin=2, maxiter=8)
    got = [(s.adapt.warmup, s.adapt.target, s.adapt.burn, s.adapt.thin, s.adapt.rows) for s in seen[4:]]
    assert got == [(3, 0.234, 3, 1, 2), (3, 0.44, 3, 1, 2), (3, 0.65, 3, 2, 1), (2, 0.8, 0, 1, 5), (0, 0.234, 0, 2, 4)]


def test_abi(sa):
    """Declared in the header, exported, bound, with the argument types of the declaration; the struct mirrors the library's."""
    from stochopy_amd import _lib

    header = open(os.path.join(ROOT, "include", "stochopy_hip.h")).read()
    lib = _lib.lib()
    vp, i64, f64 = C.c_void_p, C.c_int64, C.c_double
    a, ad = C.POINTER(_lib.SxSampleArgs), C.POINTER(_lib.SxSampleAdapt)
    want = {
        "sx_sample_adapt_bytes": ([], "void"),
        "sx_sample_run_adapt": ([a, ad, i64, i64, vp], "const sx_sample_args *a, const sx_sample_adapt *ad, int64_t it0, "
                                "int64_t steps, void *stream"),
        "sx_sample_propose_adapt": ([a, ad, i64, vp, vp, vp, vp], "const sx_sample_args *a, const sx_sample_adapt *ad, "
                                    "int64_t it, double *prop, double *pmom, double *k0, void *stream"),
        "sx_sample_leap_adapt": ([a, ad, f64, C.c_int, vp, vp, vp, vp], "const sx_sample_args *a, const sx_sample_adapt *ad, "
                                 "double coef, int move, double *q, double *pmom, const double *G, void *stream"),
        "sx_sample_decide_adapt": ([a, ad, i64, vp, vp, vp, vp, vp], "const sx_sample_args *a, const sx_sample_adapt *ad, "
                                   "int64_t it, const double *prop, const double *fprop, const double *pmom, "
                                   "const double *k0, void *stream"),
    }
    for name, (argtypes, declared) in want.items():
        decl = re.search(r"^int " + name + r"\(([^)]*)\);", header, re.M)
        assert decl, name
        assert " ".join(decl.group(1).split()) == declared
        assert _lib.PROTOTYPES[name] == (C.c_int, argtypes)
        assert getattr(lib, name).argtypes == argtypes and getattr(lib, name).restype is C.c_int
    # the new forms take the old ones' arguments with `ad` behind `a`
    for name in ("run", "propose", "leap", "decide"):
        old = _lib.PROTOTYPES["sx_sample_" + name][1]
        assert _lib.PROTOTYPES[f"sx_sample_{name}_adapt"][1] == [old[0], ad] + old[1:]
    assert C.sizeof(_lib.SxSampleAdapt) == lib.sx_sample_adapt_bytes() == 72
    fields = re.search(r"typedef struct sx_sample_adapt \{(.*?)\} sx_sample_adapt;", header, re.S).group(1)
    names = re.findall(r"\*?(\w+)\s*[,;]", re.sub(r"/\*.*?\*/", "", fields, flags=re.S))
    assert names == [f[0] for f in _lib.SxSampleAdapt._fields_]
    # sx_sample_args and sx_struct_size are what they were
    assert lib.sx_struct_size(7) == C.sizeof(_lib.SxSampleArgs) == 208 and lib.sx_struct_size(13) == -1
    # the constants of the rule are named where the kernels share them
    hpp = open(os.path.join(ROOT, "stochopy_amd", "csrc", "sx_sample.hpp")).read()
    for text in ("kAdaptT0 = 10.0", "kAdaptGamma = 0.05", "kAdaptLogMu = 2.302585092994046"):
        assert text in hpp
    assert float.fromhex(float(np.log(10.0)).hex()) == 2.302585092994046


def test_the_library_checks_its_arguments(sa):
    """The SX_REQUIRE checks of the *_adapt entry points fail on the host, before any launch."""
    from stochopy_amd import _lib

    lib = _lib.lib()
    a, ad = _lib.SxSampleArgs(), _lib.SxSampleAdapt()
    for name in ("cur", "fcur", "facc", "fmin", "xbest", "iacc", "imin", "nacc", "nfeas", "lower", "upper", "step"):
        setattr(a, name, 8)  # (never dereferenced: every call below is refused)
    a.C, a.maxiter, a.n, a.k, a.nleap = 2, 10, 4, 4, 1
    a.method, a.rng, a.jac = _lib.SX_SAMPLE_MCMC, _lib.SX_RNG_PHILOX, _lib.SX_JAC_ANALYTIC

    def refused(text, **fields):
        good = {"warmup": 0, "rec_start": 0, "rec_every": 1, "rec_rows": 10, "target": 0.234,
                "scale": None, "hbar": None, "logsbar": None, "nacc_warm": None}
        for key, value in dict(good, **fields).items():
            setattr(ad, key, value)
        assert lib.sx_sample_run_adapt(C.byref(a), C.byref(ad), 0, 1, None) == -1
        assert text in lib.sx_last_error().decode(), lib.sx_last_error()
        assert lib.sx_sample_decide_adapt(C.byref(a), C.byref(ad), 0, 8, 8, None, None, None) == -1
        assert text in lib.sx_last_error().decode(), lib.sx_last_error()

    refused("warmup", warmup=-1)
    refused("warmup", warmup=10)
    refused("rec_start", rec_start=10, rec_rows=0)
    refused("rec_start", rec_start=-1, rec_rows=11)
    refused("rec_every", rec_every=0)
    refused("rec_every", rec_every=1 << 31, rec_rows=1)
    refused("rec_rows", rec_rows=9)
    refused("rec_rows", rec_start=3, rec_every=3, rec_rows=2)  # ceil(7 / 3) = 3
    refused("null adaptation state", warmup=3)
    refused("target", warmup=3, scale=8, hbar=8, logsbar=8, nacc_warm=8, target=1.0)
    refused("target", warmup=3, scale=8, hbar=8, logsbar=8, nacc_warm=8, target=float("nan"))
    a.rng = _lib.SX_RNG_HOST
    a.C, a.x0, a.normals, a.logu = 1, 8, 8, 8
    refused("SX_RNG_PHILOX")
    assert lib.sx_sample_run_adapt(C.byref(a), None, 0, 1, None) == -1


@pytest.mark.parametrize("method,objective,ndim,chains,options,burn,thin", [
    ("mcmc", "rastrigin", 5, 3, {"stepsize": 0.05, "perc": 0.5}, 7, 3),
    ("mcmc", "sphere", 70, 1, {"stepsize": 0.05, "perc": 0.3, "constraints": "Reject"}, 0, 4),
    ("hmc", "sphere", 4, 2, {"stepsize": 0.01, "nleap": 3, "jac": "analytic"}, 11, 1),
    ("hmc", "styblinski_tang", 3, 5, {"stepsize": 0.01, "nleap": 2, "jac": None}, 29, 50),
])
def test_without_a_warmup_the_oracle_is_the_plain_one_thinned(method, objective, ndim, chains, options, burn, thin):
    bounds = [[-5.12, 5.12]] * ndim
    o = dict(options, maxiter=30, seed=9, chains=chains)
    with np.errstate(all="ignore"):
        want = _sample_oracle.sample(objective, bounds, method=method, options=dict(o, rng="philox"))
    got = _sample_adapt_oracle.sample(objective, bounds, method=method, options=dict(o, warmup=0, burn=burn, thin=thin))
    wx, wf = (want.xall[None], want.funall[None]) if chains == 1 else (want.xall, want.funall)
    gx, gf = (got.xall[None], got.funall[None]) if chains == 1 else (got.xall, got.funall)
    assert gx.shape == (chains, -(-(30 - burn) // thin), ndim)
    assert np.array_equal(gx, wx[:, burn::thin]) and np.array_equal(gf, wf[:, burn::thin])
    assert np.array_equal(got.x, want.x) and got.fun == want.fun and got.accept_ratio == want.accept_ratio
    assert np.array_equal(got.nacc, want.nacc) and np.array_equal(got.nfeas, want.nfeas)
    assert "stepsizes" not in got and "warmup" not in got
    if method == "hmc":
        assert got.nfev == want.nfev


@functools.lru_cache(maxsize=None)
def adapted(method, stepsize, warmup=300):
    o = {"maxiter": 800, "seed": 0, "chains": 256, "stepsize": stepsize, "warmup": warmup, "burn": 300}
    if method == "hmc":
        o["jac"] = "analytic"
    return _sample_adapt_oracle.sample("sphere", [[-5.0, 5.0]] * 8, method=method, options=o)


# (method, the two starting steps, the band of the mean acceptance, and what the prototype of the rule measured: mean
# acceptance, pooled variance and mean effective step of either run)
TABLE = [("mcmc", (0.5, 0.001), (0.15, 0.30), ((0.194, 0.503, 0.1426), (0.205, 0.502, 0.1392))),
         ("hmc", (0.2, 0.0005), (0.6, 0.95), ((0.756, 0.504, 0.1598), (0.807, 0.498, 0.1578)))]


@pytest.mark.parametrize("method,steps,accept_band,measured", TABLE)
def test_the_oracle_adapts(method, steps, accept_band, measured):
    """sphere, ndim 8, bounds +-5, 256 chains, seed 0, 800 samples of which 300 adapt: exp(-sum x^2) has variance 0.5 per
    component.  From two starting steps two or more orders of magnitude apart the chains end at the same step, the
    acceptance is near its target and the variance over samples 300 ... 799 is right -- the bands the GPU test asserts."""
    runs = [adapted(method, s) for s in steps]
    effective = []
    for s, r, (m_accept, m_var, m_step) in zip(steps, runs, measured):
        accept, var = float(r.accept_ratios_sampling.mean()), float(r.xall.var())
        effective.append(float((r.stepsizes * s).mean()))
        print(method, "stepsize", s, "acceptance", accept, "pooled variance", var, "effective step", effective[-1],
              "chains", float((r.stepsizes * s).min()), "...", float((r.stepsizes * s).max()))
        assert r.xall.shape == (256, 500, 8) and r.warmup == 300
        assert accept_band[0] <= accept <= accept_band[1]
        assert 0.45 <= var <= 0.55
        assert np.all(np.isfinite(r.stepsizes)) and np.all(r.stepsizes > 0.0)
        # the restatement is the prototype's rule: its figures to the digits they were reported with
        assert abs(accept - m_accept) < 1e-3 and abs(var - m_var) < 1e-3 and abs(effective[-1] - m_step) < 1e-4
    assert 0.9 <= effective[0] / effective[1] <= 1.1


@pytest.mark.parametrize("method,stepsize,wrong", [("mcmc", 0.001, 8.09), ("hmc", 0.0005, 3.99)])
def test_without_a_warmup_the_same_run_is_wrong(method, stepsize, wrong):
    """What the warm-up is for: the same chains with the guessed step have not reached the target's variance."""
    var = float(adapted(method, stepsize, warmup=0).xall.var())
    print(method, "stepsize", stepsize, "pooled variance without a warm-up", var)
    assert abs(var - wrong) < 0.05 * wrong
