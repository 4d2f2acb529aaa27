"""No GPU: per-axis scale adaptation in the warm-up for stochopy_amd.sample (metric="diag") -- the option's validation (every
refusal is raised before the device is touched), the window schedule, the C ABI additions, and the numpy restatement
(tests/_sample_metric_oracle.py): its link to the restatement of the scalar warm-up and the statistical claim the GPU test
relies on."""
import ctypes as C
import functools
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _sample_adapt_oracle  # noqa: E402
import _sample_metric_cases as cases  # noqa: E402
import _sample_metric_oracle  # noqa: E402

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
    o = dict({"rng": "philox", "chains": 2, "maxiter": 30, "seed": 1}, **options)
    return sa.sample.sample(sa.factory.sphere, [[-5.12, 5.12]] * ndim, method=method, options=o)


REFUSALS = [
    ({"metric": "diag"}, ValueError),                                             # no warm-up
    ({"metric": "diag", "warmup": 19}, ValueError),                               # 20 is the least
    ({"metric": "diag", "burn": 3, "thin": 2}, ValueError),                       # burn / thin alone are no warm-up
    ({"metric": "diag", "warmup": 20, "rng": "numpy-legacy", "chains": 1}, ValueError),
    ({"metric": "dense", "warmup": 20}, ValueError),
    ({"metric": "", "warmup": 20}, ValueError),
    ({"metric": "Diag", "warmup": 20}, ValueError),
    ({"metric": 1, "warmup": 20}, TypeError),
    ({"metric": True, "warmup": 20}, TypeError),
    ({"metric": ["diag"], "warmup": 20}, TypeError),
    ({"metric": np.ones(4), "warmup": 20}, TypeError),
]


@pytest.mark.parametrize("method", ["mcmc", "hmc"])
@pytest.mark.parametrize("options,error", REFUSALS)
def test_refusals_name_metric_and_come_before_the_device(sa, no_device, method, options, error):
    with pytest.raises(error, match="metric"):
        call(sa, method=method, **options)


def test_refused_with_temperatures(sa, no_device):
    for extra in ({}, {"swap_every": 2}):
        with pytest.raises(ValueError, match="metric"):
            call(sa, temperatures=[1.0, 2.0, 4.0], metric="diag", **extra)
        with pytest.raises(ValueError, match="metric"):
            call(sa, method="hmc", temperatures=[1.0, 2.0, 4.0], metric="diag", **extra)
    # the refusals that were there stay what they were, and come first
    with pytest.raises(ValueError, match="warmup"):
        call(sa, temperatures=[1.0, 2.0, 4.0], metric="diag", warmup=20)
    with pytest.raises(ValueError, match="mcmc"):
        call(sa, method="hmc", temperatures=[1.0, 2.0, 4.0])
    with pytest.raises(ValueError, match="mcmc"):
        call(sa, method="hmc", temperatures=[1.0, 2.0, 4.0], metric=None)


def test_the_other_errors_come_first(sa, no_device):
    with pytest.raises(ValueError) as e:  # (bounds that are no (ndim, 2) array: the reference's bare ValueError)
        sa.sample.sample(sa.factory.sphere, [1.0, 2.0], method="mcmc", options={"rng": "philox", "metric": 3})
    assert str(e.value) == ""
    with pytest.raises(ValueError) as e:
        call(sa, perc=1.5, metric=3)
    assert str(e.value) == ""
    with pytest.raises(ValueError) as e:
        call(sa, method="hmc", nleap=0, metric=3)
    assert str(e.value) == ""
    with pytest.raises(TypeError, match="warmup"):  # the warm-up's own checks, then metric's
        call(sa, warmup="x", metric=3)


def test_accepted_values_pass_the_checks_and_the_default_changes_nothing(sa, no_device, monkeypatch):
    for method in ("mcmc", "hmc"):
        with pytest.raises(AssertionError, match="the device was touched"):
            call(sa, method=method, metric="diag", warmup=20)
        with pytest.raises(AssertionError, match="the device was touched"):
            call(sa, method=method, metric="diag", warmup=29, burn=0, thin=2, target_accept=0.8)
    from stochopy_amd.sample import _chains

    seen = []
    monkeypatch.setattr(_chains, "run", lambda s: seen.append(s) or "ran")
    for method in ("mcmc", "hmc"):
        assert call(sa, method=method) == "ran" and call(sa, method=method, metric=None) == "ran"
        assert call(sa, method=method, warmup=25, metric=None) == "ran"
        assert call(sa, method=method, warmup=25, metric="diag") == "ran"
    plain, same, adapting, scaled = seen[:4]
    assert plain.adapt is None and same.adapt is None and adapting.adapt.windows is None
    assert all(s.adapt.windows == (3, (23,)) and s.adapt.warmup == 25 for s in (scaled, seen[7]))
    # `metric` stands behind `thin`: positional calls are what they were
    import inspect

    for fn in (sa.sample.mcmc, sa.sample.hmc):
        names = list(inspect.signature(fn).parameters)
        assert names[-2:] == ["thin", "metric"] and inspect.signature(fn).parameters["metric"].default is None


@pytest.mark.parametrize("warmup,start,ends", [
    (20, 3, (18,)),                 # span 15: one window (15 // 3 = 5 < 8)
    (40, 6, (16, 36)),              # span 30: 30 // 3 = 10 -> windows of 10 and 20
    (600, 90, (120, 180, 300, 540)),     # span 450: 450 // 15 = 30 -> 30, 60, 120, 240
    (1000, 150, (200, 300, 500, 900)),   # span 750: 750 // 15 = 50 -> 50, 100, 200, 400
])
def test_the_schedule(sa, warmup, start, ends):
    from stochopy_amd.sample import _adapt

    assert _adapt.metric_windows(warmup) == (start, ends)
    assert _sample_metric_oracle.windows(warmup) == (start, ends)


def test_the_schedule_everywhere(sa):
    from stochopy_amd.sample import _adapt

    for W in range(20, 3000):
        start, ends = _adapt.metric_windows(W)
        assert (start, ends) == _sample_metric_oracle.windows(W)
        edges = (start,) + ends
        assert 1 <= len(ends) <= 4 and start >= 3 and ends[-1] == W - (10 * W) // 100 <= W
        lengths = np.diff(edges)
        assert np.all(lengths >= 8) and np.all(lengths[1:] >= lengths[:-1])


def test_abi(sa):
    """Declared in the header, exported, bound, with the argument types of the declaration; the struct mirrors the library's."""
    from stochopy_amd import _lib

    header = open(os.path.join(ROOT, "include", "stochopy_hip.h")).read()
    lib = _lib.lib()
    mt = C.POINTER(_lib.SxSampleMetric)
    assert _lib.PROTOTYPES["sx_sample_metric_bytes"] == (C.c_int, [])
    for name in ("run", "propose", "leap", "decide"):  # the *_adapt forms' arguments with `mt` behind `ad`
        old = _lib.PROTOTYPES[f"sx_sample_{name}_adapt"][1]
        new = f"sx_sample_{name}_metric"
        assert _lib.PROTOTYPES[new] == (C.c_int, old[:2] + [mt] + old[2:])
        assert getattr(lib, new).argtypes == old[:2] + [mt] + old[2:] and getattr(lib, new).restype is C.c_int
        decl = re.search(r"^int " + new + r"\(([^)]*)\);", header, re.M)
        was = re.search(r"^int sx_sample_" + name + r"_adapt\(([^)]*)\);", header, re.M)
        assert " ".join(decl.group(1).split()) == " ".join(was.group(1).split()).replace(
            "const sx_sample_adapt *ad,", "const sx_sample_adapt *ad, const sx_sample_metric *mt,")
    assert C.sizeof(_lib.SxSampleMetric) == lib.sx_sample_metric_bytes() == 4 * 8 + 8 + 8 + 8 * 8
    fields = re.search(r"typedef struct sx_sample_metric \{(.*?)\} sx_sample_metric;", header, re.S).group(1)
    names = re.findall(r"\*?(\w+)\s*(?:\[8\])?\s*[,;]", re.sub(r"/\*.*?\*/", "", fields, flags=re.S))
    assert names == [f[0] for f in _lib.SxSampleMetric._fields_] == ["sbase", "m", "mean", "M2", "nwin", "win_start", "win_end"]
    # the structs that were there are what they were
    assert lib.sx_struct_size(7) == C.sizeof(_lib.SxSampleArgs) == 208 and lib.sx_sample_adapt_bytes() == 72
    readme = open(os.path.join(ROOT, "README.md")).read()
    declared = set(re.findall(r"\b(sx_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    assert f"({len(declared)} entry points" in readme


def test_the_library_checks_its_arguments(sa):
    """The SX_REQUIRE checks of the *_metric entry points fail on the host, before any launch."""
    from stochopy_amd import _lib

    lib = _lib.lib()
    a, ad, mt = _lib.SxSampleArgs(), _lib.SxSampleAdapt(), _lib.SxSampleMetric()
    for name in ("cur", "fcur", "facc", "fmin", "xbest", "iacc", "imin", "nacc", "nfeas", "lower", "upper", "step"):
        setattr(a, name, 8)  # (never dereferenced: every call below is refused)
    a.C, a.maxiter, a.n, a.k, a.nleap = 2, 50, 4, 4, 1
    a.method, a.rng, a.jac = _lib.SX_SAMPLE_MCMC, _lib.SX_RNG_PHILOX, _lib.SX_JAC_ANALYTIC
    for name in ("scale", "hbar", "logsbar", "nacc_warm"):
        setattr(ad, name, 8)
    ad.warmup, ad.rec_start, ad.rec_every, ad.rec_rows, ad.target = 40, 0, 1, 50, 0.234

    def refused(text, nwin, start=6, ends=(), pointers=8):
        for name in ("sbase", "m", "mean", "M2"):
            setattr(mt, name, pointers)
        mt.nwin, mt.win_start = nwin, start
        for j in range(8):
            mt.win_end[j] = ends[j] if j < len(ends) else 0
        assert lib.sx_sample_run_metric(C.byref(a), C.byref(ad), C.byref(mt), 0, 1, None) == -1
        assert text in lib.sx_last_error().decode(), lib.sx_last_error()
        assert lib.sx_sample_decide_metric(C.byref(a), C.byref(ad), C.byref(mt), 0, 8, 8, None, None, None) == -1
        assert text in lib.sx_last_error().decode(), lib.sx_last_error()

    refused("nwin", -1)
    refused("nwin", 9)
    refused("null metric state", 1, ends=(16,), pointers=None)
    refused("win_start", 1, start=-1, ends=(16,))
    refused("do not increase", 2, ends=(16, 16))
    refused("do not increase", 1, start=16, ends=(16,))
    refused("do not increase", 3, ends=(16, 36, 30))
    refused("after the warm-up", 2, ends=(16, 41))
    assert lib.sx_sample_run_metric(C.byref(a), C.byref(ad), None, 0, 1, None) == -1
    assert "null metric args" in lib.sx_last_error().decode()
    ad.warmup = 50  # the checks of `ad` come first
    refused("warmup", 1, ends=(16,))


@pytest.mark.parametrize("method,objective,ndim,chains,options", [
    ("mcmc", "rastrigin", 5, 3, {"stepsize": 0.05, "perc": 0.5, "warmup": 25, "burn": 7, "thin": 3}),
    ("mcmc", "sphere", 70, 1, {"stepsize": 0.05, "perc": 0.3, "constraints": "Reject", "warmup": 29}),
    ("hmc", "sphere", 4, 2, {"stepsize": 0.01, "nleap": 3, "jac": "analytic", "warmup": 20, "target_accept": 0.8}),
    ("hmc", "styblinski_tang", 3, 5, {"stepsize": 0.01, "nleap": 2, "jac": None, "warmup": 12, "burn": 0}),
])
def test_with_no_window_the_oracle_is_the_adapting_one(method, objective, ndim, chains, options):
    bounds = [[-5.12, 5.12]] * ndim
    o = dict(options, maxiter=30, seed=9, chains=chains)
    want = _sample_adapt_oracle.sample(objective, bounds, method=method, options=dict(o))
    for extra in ({}, {"metric": None}, {"windows": (5, ())}):
        got = _sample_metric_oracle.sample(objective, bounds, method=method, options=dict(o, **extra))
        assert set(got) == set(want)
        for key in want:
            assert np.array_equal(got[key], want[key], equal_nan=True), key
    assert not np.all(want.stepsizes == 1.0)


@functools.lru_cache(maxsize=None)
def gauss(method, seed, metric):
    o = cases.gauss_options(method, seed, metric)
    if method == "hmc":
        o["jac"] = cases.gauss_gradient
    return _sample_metric_oracle.sample(cases.gauss_value, cases.GAUSS_BOUNDS, x0=np.zeros(8), method=method, options=o)


@pytest.mark.parametrize("seed", cases.GAUSS_SEEDS)
@pytest.mark.parametrize("method", ["mcmc", "hmc"])
def test_the_oracle_adapts_per_axis(method, seed):
    """The anisotropic Gaussian of tests/_sample_metric_cases.py: with the scalar warm-up the step settles on the narrowest
    axis and the widest moves by a tiny fraction of its width per sample; with the scales every axis moves.  The bound on the
    ratio is half the smallest of the five ratios measured on this restatement (profiles/sample_metric_cases.txt)."""
    scalar, scaled = gauss(method, seed, None), gauss(method, seed, "diag")
    slow, fast = cases.slowest_jump(scalar.xall), cases.slowest_jump(scaled.xall)
    learnt = float(np.mean(scaled.metric[:, -1] / scaled.metric[:, 0]))
    print(method, "seed", seed, "slowest axis: scalar", slow, "with the scales", fast, "ratio", fast / slow, "learnt", learnt)
    assert scaled.metric.shape == (cases.GAUSS_CHAINS, 8) and scaled.metric_windows == _sample_metric_oracle.windows(
        cases.GAUSS[method]["warmup"])[1]
    assert fast / slow >= cases.GAUSS_RATIO_BOUND[method]
    assert cases.SCALE_RATIO_EXACT / 2 <= learnt <= cases.SCALE_RATIO_EXACT * 2
    assert np.allclose(np.exp(np.log(scaled.metric).mean(axis=1)), 1.0, rtol=1e-12)  # geometric mean 1: s keeps its meaning
