"""No GPU: parallel tempering for stochopy_amd.sample (method="mcmc", options temperatures / swap_every) -- the options'
validation (every refusal is raised before the device is touched), the C ABI additions, and the numpy restatement
(tests/_temper_oracle.py): its link to the plain restatement and that it samples a multimodal target correctly."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _sample_oracle  # noqa: E402
import _temper_oracle  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUNDS = [[-5.12, 5.12]] * 4
LADDER = [1.0, 2.0, 4.0]


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


@pytest.mark.parametrize("options,error", [
    ({"temperatures": [2.0, 4.0]}, ValueError),                # does not start at 1
    ({"temperatures": [1.0]}, ValueError),                     # K < 2
    ({"temperatures": []}, ValueError),
    ({"temperatures": [1.0, 2.0, 2.0]}, ValueError),           # not strictly increasing
    ({"temperatures": [1.0, 3.0, 2.0]}, ValueError),
    ({"temperatures": [1.0, np.inf]}, ValueError),
    ({"temperatures": [1.0, np.nan]}, ValueError),
    ({"temperatures": [[1.0, 2.0]]}, ValueError),              # not 1-D
    ({"temperatures": 2.0}, TypeError),
    ({"temperatures": "1,2"}, TypeError),
    ({"temperatures": [1.0, "hot"]}, TypeError),
    ({"temperatures": LADDER, "swap_every": 0}, ValueError),
    ({"temperatures": LADDER, "swap_every": -3}, ValueError),
    ({"temperatures": LADDER, "swap_every": 2.0}, TypeError),
    ({"temperatures": LADDER, "swap_every": True}, TypeError),
    ({"swap_every": 2}, ValueError),                           # swap_every without temperatures
    ({"temperatures": LADDER, "rng": "numpy-legacy", "chains": 1}, ValueError),
    ({"temperatures": LADDER, "rng": "numpy-legacy"}, ValueError),
])
def test_refusals_name_temperatures_and_come_before_the_device(sa, no_device, options, error):
    with pytest.raises(error, match="temperatures"):
        call(sa, **options)


def test_hmc_is_refused(sa, no_device):
    with pytest.raises(ValueError, match="temperatures"):
        call(sa, method="hmc", temperatures=LADDER)
    with pytest.raises(ValueError, match="temperatures"):
        call(sa, method="hmc", swap_every=2)


def test_too_many_rungs_are_refused(sa, no_device):
    from stochopy_amd import _lib

    L = _lib.lib()
    for ndim, want in ((1, 16), (64, 16), (128, 16), (129, 8), (1024, 8), (2048, 4)):
        assert L.sx_sample_tempered_max_rungs(ndim) == want
    assert L.sx_sample_tempered_max_rungs(0) == -1 and L.sx_sample_tempered_max_rungs(_lib.wide_from() + 1) == -1
    for ndim in (4, 200, 2048):
        most = L.sx_sample_tempered_max_rungs(ndim)
        with pytest.raises(ValueError, match="temperatures"):
            call(sa, ndim=ndim, temperatures=np.arange(1.0, most + 2.0))
        with pytest.raises(AssertionError, match="the device was touched"):  # (K = most passes every check)
            call(sa, ndim=ndim, temperatures=np.arange(1.0, most + 1.0))


def test_max_rungs_is_what_fits_a_workgroup():
    """K rows of n + gen_row_stride(n) doubles fit the 160 KiB of a workgroup next to the 16 published values, and the
    workgroup's row limit: 16 rows, 8 wavefronts of 64 / lanes_per_row(n) rows."""
    from stochopy_amd import _lib

    L = _lib.lib()
    for n in (1, 64, 65, 128, 129, 256, 257, 700, 1024, 2048):
        lpr = 16 if n <= 64 else 32 if n <= 128 else 64
        K = L.sx_sample_tempered_max_rungs(n)
        assert 2 <= K <= min(16, 8 * (64 // lpr))
        if n <= 256:
            assert K * (2 * n + 8) * 8 + 128 <= 160 * 1024
        assert K * 2 * n * 8 <= 160 * 1024


def test_abi(sa):
    """Declared in the header, exported, bound, with the argument types of the declaration."""
    from stochopy_amd import _lib

    header = open(os.path.join(ROOT, "include", "stochopy_hip.h")).read()
    lib = _lib.lib()
    vp, i64 = C.c_void_p, C.c_int64
    args = C.POINTER(_lib.SxSampleArgs)
    want = {
        "sx_sample_tempered_run": [args, vp, C.c_int, i64, vp, i64, i64, vp],
        "sx_sample_tempered_max_rungs": [C.c_int],
        "sx_sample_decide_tempered": [args, i64, vp, vp, vp, C.c_int, C.c_int, vp],
        "sx_sample_swap": [args, i64, i64, vp, C.c_int, vp, vp],
    }
    for name, argtypes in want.items():
        assert re.search(r"^int " + name + r"\(", header, re.M), name
        assert _lib.PROTOTYPES[name] == (C.c_int, argtypes)
        assert getattr(lib, name).argtypes == argtypes and getattr(lib, name).restype is C.c_int
    decl = re.search(r"int sx_sample_tempered_run\(([^)]*)\)", header).group(1)
    assert [" ".join(p.split()) for p in decl.split(",")] == [
        "const sx_sample_args *a", "const double *beta", "int K", "int64_t swap_every", "int64_t *nswap", "int64_t it0",
        "int64_t steps", "void *stream"]
    assert "kPurposeSampleSwap = 14" in open(os.path.join(ROOT, "stochopy_amd", "csrc", "sx_device.hpp")).read()
    # sx_sample_args and sx_struct_size are what they were
    assert lib.sx_struct_size(7) == C.sizeof(_lib.SxSampleArgs) and lib.sx_struct_size(13) <= 0


def test_without_temperatures_the_call_path_is_untouched(sa, monkeypatch):
    from stochopy_amd.sample import _chains, _temper

    seen = []
    monkeypatch.setattr(_chains, "run", lambda s: seen.append(s) or "plain")
    monkeypatch.setattr(_temper, "run", lambda s: pytest.fail("the tempered path ran"))
    assert call(sa) == "plain" and call(sa, temperatures=None, swap_every=None) == "plain"
    assert all(s.temperatures is None and s.swap_every is None and s.chains == 2 for s in seen) and len(seen) == 2
    monkeypatch.setattr(_temper, "run", lambda s: ("tempered", s))
    tag, s = call(sa, temperatures=LADDER)
    assert tag == "tempered" and s.swap_every == 1 and np.array_equal(s.temperatures, LADDER) and len(seen) == 2
    assert s.temperatures.dtype == np.float64 and s.chains == 2 and s.k == 4


@pytest.mark.parametrize("objective,ndim,perc,constraints,x0", [
    ("sphere", 3, 1.0, None, None),
    ("rastrigin", 5, 0.5, "Reject", "shared"),
    ("rosenbrock", 70, 0.3, None, "per-ladder"),
])
def test_without_events_the_cold_rung_is_the_plain_chain(objective, ndim, perc, constraints, x0):
    """swap_every > maxiter: rung 0 of ladder c is chain c K of the plain restatement with C K chains, bit for bit."""
    Cn, K, m = 3, 4, 25
    bounds = [[-5.12, 5.12]] * ndim
    rs = np.random.RandomState(3)
    start = {None: None, "shared": rs.uniform(-2, 2, ndim), "per-ladder": rs.uniform(-2, 2, (Cn, ndim))}[x0]
    opts = {"maxiter": m, "stepsize": 0.3 if constraints else 0.05, "perc": perc, "seed": 77, "constraints": constraints}
    got = _temper_oracle.sample(objective, bounds, [1.0, 1.5, 4.0, 9.0], x0=start,
                                options=dict(opts, chains=Cn, swap_every=m + 1), keep_hot=True)
    plain_x0 = np.repeat(start, K, axis=0) if x0 == "per-ladder" else start
    with np.errstate(all="ignore"):
        want = _sample_oracle.sample(objective, bounds, x0=plain_x0, method="mcmc",
                                     options=dict(opts, chains=Cn * K, rng="philox"))
    assert np.array_equal(got.xall, want.xall[::K]) and np.array_equal(got.funall, want.funall[::K])
    assert np.array_equal(got.nacc[:, 0], want.nacc[::K]) and np.array_equal(got.nfeas[:, 0], want.nfeas[::K])
    assert np.all(got.nswap == 0) and np.all(got.swap_ratios == 0.0)
    assert 0 < got.nacc[:, 0].sum() < Cn * m
    assert np.array_equal(got.xall_replicas[:, 0], want.xall[:, 0])  # the hot rungs start where the plain chains start


def test_the_oracle_exchanges_as_specified():
    """The events a pair takes part in by parity, the counts and ratios, and nothing is exchanged before the first event."""
    Cn, K, m, every = 2, 5, 41, 3
    got = _temper_oracle.sample("rastrigin", BOUNDS, np.geomspace(1.0, 30.0, K), options={
        "maxiter": m, "seed": 5, "chains": Cn, "swap_every": every, "stepsize": 0.05}, keep_hot=True)
    attempts = _temper_oracle.swap_attempts(K, m, every)
    assert attempts.tolist() == [7, 6, 7, 6]  # events 1 .. 13: seven odd, six even
    assert np.array_equal(got.swap_ratios, got.nswap / attempts) and got.nswap.sum() > 0
    assert got.accept_ratios.shape == (Cn, K) and got.swap_ratios.shape == (Cn, K - 1)
    X = got.xall_replicas
    # identical to the run without events until the first event
    res2 = _temper_oracle.sample("rastrigin", BOUNDS, np.geomspace(1.0, 30.0, K), options={
        "maxiter": m, "seed": 5, "chains": Cn, "swap_every": m + 1, "stepsize": 0.05}, keep_hot=True)
    assert np.array_equal(res2.xall_replicas[:, :every], X[:, :every])
    assert not np.array_equal(res2.xall_replicas[:, every], X[:, every])


def rastrigin_mass():
    """The mass of exp(-rastrigin) on |x| < 0.5 within [-5.12, 5.12], by the trapezoid rule on 2^21 intervals."""
    x = np.linspace(-5.12, 5.12, (1 << 21) + 1)
    p = np.exp(-(10.0 + x * x - 10.0 * np.cos(2.0 * np.pi * x)))
    w = np.full(x.size, x[1] - x[0])
    w[0] = w[-1] = 0.5 * (x[1] - x[0])
    return float((p * w)[np.abs(x) < 0.5].sum() / (p * w).sum())


TARGET = {"bounds": [[-5.12, 5.12]], "x0": np.array([3.0]), "ladder": np.geomspace(1.0, 32.0, 8),
          "options": {"maxiter": 8000, "stepsize": 0.03, "constraints": "Reject", "swap_every": 2}}


def cold_share(xall):
    """The share of cold samples with |x| < 0.5 over samples maxiter // 2 ..., taken every 10th."""
    m = xall.shape[1]
    return float(np.mean(np.abs(xall[:, m // 2::10, 0]) < 0.5))


@pytest.mark.parametrize("seed", [11, 12, 13])
def test_the_oracle_samples_a_multimodal_target(seed):
    """1-D rastrigin as -log p: modes at the integers, barriers ~20 high.  All replicas start at x = 3.  The tempered
    cold rungs spend the exact share of their time in the central well (within 0.03: five times the +-0.006 a plain
    numpy simulation of the algorithm spread over six seeds); the same replicas without tempering never get there.
    128 ladders (the 256 of the simulation take twice as long; the spread of the share over the seeds is printed)."""
    want = rastrigin_mass()
    assert abs(want - 0.5626) < 1e-3
    o = dict(TARGET["options"], seed=seed, chains=128)
    got = _temper_oracle.sample("rastrigin", TARGET["bounds"], TARGET["ladder"], x0=TARGET["x0"], options=o)
    share = cold_share(got.xall)
    print("seed", seed, "share", share, "exact", want, "lowest swap ratio", got.swap_ratios.min())
    assert abs(share - want) <= 0.03
    assert np.all(got.swap_ratios > 0.3) and np.all(got.swap_ratios < 1.0)
    o.pop("swap_every")
    with np.errstate(all="ignore"):
        plain = _sample_oracle.sample("rastrigin", TARGET["bounds"], x0=TARGET["x0"], method="mcmc",
                                      options=dict(o, chains=128 * 8, rng="philox"))
    assert cold_share(plain.xall) == 0.0
