"""No GPU: the moves of the ensemble sampler (method="ensemble" with ``moves`` / ``burn`` / ``thin``) -- the options' validation
(every refusal is raised before the device is touched), the C ABI additions and the library's own argument checks, and the numpy
restatement (tests/_ensemble_moves_oracle.py): its structure, that each move samples the rotated Gaussian correctly, and that
the differential-evolution move finds the weights of two separated modes where the stretch move does not."""
import ctypes as C
import functools
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _ensemble_moves_cases as cases  # noqa: E402
import _ensemble_moves_oracle as oracle  # noqa: E402
import _ensemble_oracle  # noqa: E402

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


def call(sa, ndim=3, fun=None, x0=None, callback=None, **options):
    o = dict({"chains": 2, "maxiter": 5, "seed": 1}, **options)
    return sa.sample.sample(sa.factory.sphere if fun is None else fun, [[-5.12, 5.12]] * ndim, x0=x0, method="ensemble",
                            options=o, callback=callback)


@pytest.mark.parametrize("options,error,names", [
    ({"moves": 3}, TypeError, "moves"),
    ({"moves": {"de": 1.0}}, TypeError, "moves"),
    ({"moves": []}, ValueError, "moves.*1 to 4"),
    ({"moves": ["de"] * 5}, ValueError, "moves.*1 to 4"),
    ({"moves": "walk"}, ValueError, "moves.*'walk'"),
    ({"moves": [("de", 1.0), ("kombine", 1.0)]}, ValueError, "moves.*'kombine'"),
    ({"moves": [3]}, TypeError, "moves"),
    ({"moves": [()]}, TypeError, "moves"),
    ({"moves": [("de", 1.0, 1.0, 1.0)]}, TypeError, "moves"),
    ({"moves": [(1.0, "de")]}, TypeError, "moves"),
    ({"moves": [("de", "1")]}, TypeError, "moves.*weight"),
    ({"moves": [("de", True)]}, TypeError, "moves.*weight"),
    ({"moves": [("de", 0.0)]}, ValueError, "moves.*weight"),
    ({"moves": [("de", -1.0)]}, ValueError, "moves.*weight"),
    ({"moves": [("de", np.inf)]}, ValueError, "moves.*weight"),
    ({"moves": [("de", np.nan)]}, ValueError, "moves.*weight"),
    ({"moves": [("de", 1.0), ("snooker", 1e-30)]}, ValueError, "moves.*weights"),
    ({"moves": [("stretch", 1.0, 1.0)]}, ValueError, "moves.*param.*stretch"),
    ({"moves": [("stretch", 1.0, np.inf)]}, ValueError, "moves.*param.*stretch"),
    ({"moves": [("stretch", 1.0, "2")]}, TypeError, "moves.*param.*stretch"),
    ({"moves": [("de", 1.0, 0.0)]}, ValueError, "moves.*param.*'de'"),
    ({"moves": [("de", 1.0, -0.5)]}, ValueError, "moves.*param.*'de'"),
    ({"moves": [("de", 1.0, np.nan)]}, ValueError, "moves.*param.*'de'"),
    ({"moves": [("de", 1.0, True)]}, TypeError, "moves.*param.*'de'"),
    ({"moves": [("snooker", 1.0, 0.0)]}, ValueError, "moves.*param.*snooker"),
    ({"moves": [("snooker", 1.0, np.inf)]}, ValueError, "moves.*param.*snooker"),
    ({"moves": "snooker", "ndim": 2}, ValueError, "moves.*snooker.*walkers >= 6"),        # walkers = 4
    ({"moves": [("de", 0.8), "snooker"], "ndim": 1}, ValueError, "moves.*snooker.*walkers >= 6"),
    ({"burn": 5}, ValueError, "burn"),            # maxiter - 1 = 4 is the last sample
    ({"burn": -1}, ValueError, "burn"),
    ({"burn": 1.0}, TypeError, "burn"),
    ({"burn": True}, TypeError, "burn"),
    ({"burn": "1"}, TypeError, "burn"),
    ({"thin": 0}, ValueError, "thin"),
    ({"thin": -2}, ValueError, "thin"),
    ({"thin": 2.0}, TypeError, "thin"),
    ({"thin": True}, TypeError, "thin"),
    ({"moves": "de", "rng": "numpy-legacy"}, ValueError, "rng"),
    ({"moves": "de", "seed": None}, ValueError, "seed"),
])
def test_refusals_name_the_option_and_come_before_the_device(sa, no_device, options, error, names):
    with pytest.raises(error, match=names):
        call(sa, **options)


def test_burn_and_thin_are_refused_with_the_messages_of_mcmc(sa, no_device):
    for options in ({"burn": 5}, {"burn": -1}, {"thin": 0}, {"burn": 1.5}, {"thin": "2"}):
        with pytest.raises((ValueError, TypeError)) as mine:
            call(sa, **options)
        with pytest.raises((ValueError, TypeError)) as theirs:
            sa.sample.sample(sa.factory.sphere, [[-5.12, 5.12]] * 3, method="mcmc",
                             options=dict({"maxiter": 5, "seed": 1, "rng": "philox"}, **options))
        assert type(mine.value) is type(theirs.value) and str(mine.value) == str(theirs.value)
    with pytest.raises(TypeError):  # warmup stays no option of this method
        call(sa, warmup=2, burn=2)


@pytest.mark.parametrize("options", [
    {"moves": "de"}, {"moves": "stretch"}, {"moves": "snooker"}, {"moves": ["de"]}, {"moves": ("de", "snooker")},
    {"moves": [("de", 2)]}, {"moves": [("de", np.float32(0.5), np.float64(1.0))]}, {"moves": cases.MIXTURE},
    {"moves": [("stretch", 1, 1.5), ("de", 1), ("de", 1, 1.0), ("snooker", 1, 2.0)]}, {"moves": [["de", 1.0], ["snooker", 3]]},
    {"moves": [("de", 1.0, None)]}, {"moves": "de", "ndim": 1}, {"moves": "de", "constraints": "Reject"},
    {"burn": 0}, {"burn": 4}, {"burn": np.int64(2)}, {"thin": 1}, {"thin": 3}, {"thin": 1000}, {"burn": 2, "thin": 2, "moves": "de"},
    {"moves": "de", "callback": lambda xk, state: None}, {"moves": None}])
def test_accepted_values_reach_the_device(sa, no_device, options):
    with pytest.raises(AssertionError, match="the device was touched"):
        call(sa, **options)


def test_what_the_checks_hand_to_the_run(sa, monkeypatch):
    from stochopy_amd.sample import _ensemble

    monkeypatch.setattr(_ensemble, "run", lambda s: s)
    plain = call(sa)
    assert plain.moves is None and plain.adapt is None  # the existing entry points
    s = call(sa, ndim=4, moves=cases.MIXTURE, maxiter=20, burn=7, thin=3)
    want, cum = oracle.checked_moves(cases.MIXTURE, 4)
    assert s.moves == want == [("de", 0.7 / (0.7 + 0.1 + 0.2), 2.38 / np.sqrt(8.0)), ("de", 0.1 / (0.7 + 0.1 + 0.2), 1.0),
                               ("snooker", 0.2 / (0.7 + 0.1 + 0.2), 1.7)]
    assert np.array_equal(s.cum, cum) and s.cum[-1] == 1.0 and np.all(np.diff(s.cum) > 0)
    assert (s.adapt.burn, s.adapt.thin, s.adapt.rows) == (7, 3, 5) and list(s.adapt.recorded) == [7, 10, 13, 16, 19]
    s = call(sa, moves="stretch", stretch=3.0)
    assert s.moves == [("stretch", 1.0, 3.0)] and (s.adapt.burn, s.adapt.thin, s.adapt.rows) == (0, 1, 5)
    s = call(sa, thin=2, stretch=1.5)  # burn / thin alone: the stretch move through the new entry points
    assert s.moves == [("stretch", 1.0, 1.5)] and (s.adapt.burn, s.adapt.thin, s.adapt.rows) == (0, 2, 3)
    s = call(sa, moves=[("de", 3), ("de", 1)], burn=4)
    assert [m[1] for m in s.moves] == [0.75, 0.25] and list(s.cum) == [0.75, 1.0] and s.adapt.rows == 1
    assert call(sa, thin=9).adapt.rows == 1
    assert "moves" in _ensemble.sample.__doc__ and "Out of scope" in _ensemble.sample.__doc__


def test_abi(sa):
    """Declared in the header, exported, bound, with the arguments of the existing three and the struct in the place of
    `stretch`; the struct mirrors the library's."""
    from stochopy_amd import _lib

    header = open(os.path.join(ROOT, "include", "stochopy_hip.h")).read()
    lib = _lib.lib()
    mv = C.POINTER(_lib.SxSampleEnsembleOpts)
    assert _lib.PROTOTYPES["sx_sample_ensemble_opts_bytes"] == (C.c_int, [])
    for name, was, now in (("run", "double stretch,", "const sx_sample_ensemble_opts *mv,"),
                           ("propose", "double stretch,", "const sx_sample_ensemble_opts *mv,"),
                           ("decide", "int W,", "int W, const sx_sample_ensemble_opts *mv,")):
        old = _lib.PROTOTYPES[f"sx_sample_ensemble_{name}"][1]
        new = f"sx_sample_ensemble_{name}_moves"
        argtypes = old[:2] + [mv] + old[3 if name != "decide" else 2:]
        assert _lib.PROTOTYPES[new] == (C.c_int, argtypes), new
        assert getattr(lib, new).argtypes == argtypes and getattr(lib, new).restype is C.c_int
        decl = re.search(r"^int " + new + r"\(([^)]*)\);", header, re.M)
        before = re.search(r"^int sx_sample_ensemble_" + name + r"\(([^)]*)\);", header, re.M)
        assert " ".join(decl.group(1).split()) == " ".join(before.group(1).split()).replace(was, now)
    assert C.sizeof(_lib.SxSampleEnsembleOpts) == lib.sx_sample_ensemble_opts_bytes() == 4 + 4 * 4 + 4 + 4 * 8 + 4 * 8 + 3 * 8
    fields = re.search(r"typedef struct sx_sample_ensemble_opts \{(.*?)\} sx_sample_ensemble_opts;", header, re.S).group(1)
    names = re.findall(r"\*?(\w+)\s*(?:\[4\])?\s*[,;]", re.sub(r"/\*.*?\*/", "", fields, flags=re.S))
    assert names == [f[0] for f in _lib.SxSampleEnsembleOpts._fields_] == [
        "nmoves", "kind", "cum", "param", "rec_start", "rec_every", "rec_rows"]
    assert re.search(r"SX_ENSEMBLE_STRETCH = 0, SX_ENSEMBLE_DE = 1, SX_ENSEMBLE_SNOOKER = 2", header)
    assert (_lib.SX_ENSEMBLE_STRETCH, _lib.SX_ENSEMBLE_DE, _lib.SX_ENSEMBLE_SNOOKER) == (0, 1, 2)
    device = open(os.path.join(ROOT, "stochopy_amd", "csrc", "sx_device.hpp")).read()
    assert "kPurposeSampleMove = 16" in device and "kPurposeSampleDonors = 17" in device
    assert (oracle.PURPOSE_MOVE, oracle.PURPOSE_DONORS) == (16, 17)
    # the structs that were there are what they were
    assert lib.sx_struct_size(7) == C.sizeof(_lib.SxSampleArgs) == 208 and lib.sx_sample_adapt_bytes() == 72
    readme = open(os.path.join(ROOT, "README.md")).read()
    declared = set(re.findall(r"\b(sx_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    assert {"sx_sample_ensemble_opts_bytes", "sx_sample_ensemble_run_moves", "sx_sample_ensemble_propose_moves",
            "sx_sample_ensemble_decide_moves"} <= declared
    assert f"({len(declared)} entry points" in readme


def test_the_library_checks_its_arguments(sa):
    """The checks of the *_moves entry points fail on the host, before any launch."""
    from stochopy_amd import _lib

    lib = _lib.lib()
    a, mv = _lib.SxSampleArgs(), _lib.SxSampleEnsembleOpts()
    for name in ("cur", "fcur", "facc", "fmin", "xbest", "iacc", "imin", "nacc", "nfeas", "lower", "upper"):
        setattr(a, name, 8)  # (never dereferenced: every call below is refused)
    a.C, a.maxiter, a.n = 12, 50, 2
    a.method, a.rng, a.fun_id = _lib.SX_SAMPLE_ENSEMBLE, _lib.SX_RNG_PHILOX, 0

    def refused(text, kinds=(1,), cum=(1.0,), params=(0.5,), rec=(0, 1, 50), W=6, nmoves=None):
        mv.nmoves = len(kinds) if nmoves is None else nmoves
        for k in range(4):
            mv.kind[k] = kinds[k] if k < len(kinds) else 0
            mv.cum[k] = cum[k] if k < len(cum) else 0.0
            mv.param[k] = params[k] if k < len(params) else 0.0
        mv.rec_start, mv.rec_every, mv.rec_rows = rec
        calls = (lambda: lib.sx_sample_ensemble_run_moves(C.byref(a), W, C.byref(mv), 0, 1, None),
                 lambda: lib.sx_sample_ensemble_propose_moves(C.byref(a), W, C.byref(mv), 1, 0, 8, 8, None),
                 lambda: lib.sx_sample_ensemble_decide_moves(C.byref(a), W, C.byref(mv), 1, 0, 8, 8, 8, None))
        for launch in calls:
            assert launch() == -1
            assert text in lib.sx_last_error().decode(), lib.sx_last_error()

    refused("nmoves", nmoves=0)
    refused("nmoves", nmoves=5)
    refused("unknown move kind", kinds=(3,))
    refused("unknown move kind", kinds=(1, -1), cum=(0.5, 1.0), params=(0.5, 0.5))
    refused("cum does not increase", cum=(0.0,))
    refused("cum does not increase", kinds=(1, 1), cum=(0.5, 0.5), params=(0.5, 0.5))
    refused("cum does not increase", kinds=(1, 1, 1), cum=(0.5, 0.4, 1.0), params=(0.5,) * 3)
    refused("cum does not increase", cum=(float("nan"),))
    refused("cum does not end at 1.0", cum=(0.9,))
    refused("cum does not end at 1.0", kinds=(1, 2), cum=(0.5, 1.5), params=(0.5, 0.5))
    refused("stretch entry", kinds=(0,), params=(1.0,))
    refused("stretch entry", kinds=(0,), params=(float("inf"),))
    refused("de / snooker entry", params=(0.0,))
    refused("de / snooker entry", kinds=(2,), params=(float("nan"),))
    refused("de / snooker entry", kinds=(1, 2), cum=(0.5, 1.0), params=(0.5, -1.0))
    a.C, a.n = 8, 1
    refused("snooker entry needs W >= 6", kinds=(1, 2), cum=(0.5, 1.0), params=(0.5, 0.5), W=4)
    a.C, a.n = 12, 2
    refused("rec_start", rec=(-1, 1, 51))
    refused("rec_start", rec=(50, 1, 0))
    refused("rec_every", rec=(0, 0, 50))
    refused("rec_every", rec=(0, 1 << 31, 1))
    refused("rec_rows", rec=(7, 3, 14))
    refused("rec_rows", rec=(0, 1, 49))
    # the checks of `a` come first, and a null struct is refused
    assert lib.sx_sample_ensemble_run_moves(C.byref(a), 6, None, 0, 1, None) == -1
    assert "null move options" in lib.sx_last_error().decode()
    refused("bad shape", W=5)
    a.method = _lib.SX_SAMPLE_MCMC
    refused("SX_SAMPLE_ENSEMBLE")
    a.method = _lib.SX_SAMPLE_ENSEMBLE
    assert lib.sx_sample_ensemble_run_moves(C.byref(a), 6, C.byref(mv), 49, 2, None) == -1
    assert "samples outside" in lib.sx_last_error().decode()
    a.n, a.C = 97, 194 * 2  # no resident form
    mv.nmoves, mv.kind[0], mv.cum[0], mv.param[0] = 1, 1, 1.0, 0.5
    mv.rec_start, mv.rec_every, mv.rec_rows = 0, 1, 50
    assert lib.sx_sample_ensemble_run_moves(C.byref(a), 194, C.byref(mv), 0, 1, None) == -1
    assert "does not fit the LDS" in lib.sx_last_error().decode()


# ---- the restatement's structure ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("objective,n,W,Cn,constraints,a,x0", [
    ("rastrigin", 3, 8, 4, None, 2.0, None), ("sphere", 1, 4, 2, None, 3.0, "shared"), ("rosenbrock", 8, 16, 2, "Reject", 1.5, None)])
def test_one_stretch_entry_is_the_stretch_restatement(objective, n, W, Cn, constraints, a, x0):
    bounds = [[-1.0, 1.0]] * n
    start = np.random.RandomState(n).uniform(-0.5, 0.5, (W, n)) if x0 else None
    o = {"chains": Cn, "walkers": W, "maxiter": 25, "seed": 11, "constraints": constraints}
    want = _ensemble_oracle.sample(objective, bounds, x0=start, options=dict(o, stretch=a))
    got = oracle.sample(objective, bounds, x0=start, options=dict(o, moves=[("stretch", 1, a)]))
    also = oracle.sample(objective, bounds, x0=start, options=dict(o, moves="stretch", stretch=a))
    bare = oracle.sample(objective, bounds, x0=start, options=dict(o, stretch=a))
    for key in want:
        for res in (got, also, bare):
            if key != "stretch" or res is not got:  # (got was not given the option: its a is the entry's param)
                assert np.array_equal(res[key], want[key], equal_nan=True), key
    assert got.moves == [("stretch", 1.0, a)] and (got.burn, got.thin) == (0, 1) and "moves" not in bare
    assert 0 < want.nacc.sum()


@pytest.mark.parametrize("moves", ["de", "snooker", cases.MIXTURE])
def test_the_structure_of_the_restatement(moves):
    n, W, m = 3, 8, 14
    h = W // 2
    bounds = [[-5.12, 5.12]] * n
    halves = []
    o = {"chains": 5, "walkers": W, "maxiter": m, "seed": 7, "moves": moves}
    res = oracle.sample("sphere", bounds, options=dict(o), on_half=lambda it, half, X: halves.append((it, half, X)))
    assert [(it, half) for it, half, _ in halves] == [(it, half) for it in range(1, m) for half in (0, 1)]
    moved = 0
    for it, half, X in halves:
        before = res.xall[:, it - 1] if half == 0 else halves[2 * (it - 1)][2]
        idle = slice(h, W) if half == 0 else slice(0, h)
        active = slice(0, h) if half == 0 else slice(h, W)
        assert np.array_equal(X[:, idle], before[:, idle])  # in half 0 nothing in [h, W) changes, in half 1 nothing in [0, h)
        moved += int((X[:, active] != before[:, active]).any(axis=-1).sum())
        if half == 1:
            assert np.array_equal(X, res.xall[:, it])
    assert moved == res.nacc.sum() and 0 < moved < 5 * W * (m - 1)
    # an ensemble does not depend on C
    few = oracle.sample("sphere", bounds, options=dict(o, chains=3))
    for key in ("xall", "funall", "nacc", "nfeas", "kinds"):
        assert np.array_equal(few[key], res[key][:3]), key
    one = oracle.sample("sphere", bounds, options=dict(o, chains=1))
    assert one.xall.shape == (m, W, n) and np.array_equal(one.xall, res.xall[0])
    if not isinstance(moves, str):  # one entry per ensemble and sample, every entry within 13 samples of 5 ensembles
        assert set(np.unique(res.kinds[:, 1:])) == {0, 1, 2} and np.all(res.kinds[:, 0] == -1)
        assert len({tuple(k) for k in res.kinds}) == 5  # the ensembles choose on their own
    assert res.moves == oracle.checked_moves(moves, n)[0] and abs(sum(e[1] for e in res.moves) - 1.0) < 1e-15


def test_the_entry_follows_the_weights():
    """The first k with cum[k] > u: over 4 000 (ensemble, sample) pairs the entries' shares are the weights to 3 sigma."""
    res = oracle.sample("sphere", [[-1.0, 1.0]], options={"chains": 200, "walkers": 6, "maxiter": 21, "seed": 5,
                                                           "moves": [("de", 5), ("snooker", 3), ("stretch", 2)]})
    share = np.bincount(res.kinds[:, 1:].ravel(), minlength=3) / 4000.0
    print("shares", share)
    assert np.all(np.abs(share - [0.5, 0.3, 0.2]) < 3.0 * np.sqrt(0.25 / 4000.0))


def test_the_partners_are_distinct_and_cover_every_admissible_choice():
    rs = np.random.RandomState(0)
    d0, d1, d2 = rs.random_sample((3, 20000))
    for h in (2, 3, 4, 7, 20):
        j1, j2, j3 = oracle.partners(d0, d1, d2, h, h >= 3)
        assert np.all((0 <= j1) & (j1 < h) & (0 <= j2) & (j2 < h) & (j1 != j2))
        assert len(set(zip(j1, j2))) == h * (h - 1)  # every ordered pair
        if h >= 3:
            assert np.all((0 <= j3) & (j3 < h) & (j3 != j1) & (j3 != j2))
            triples = set(zip(j1, j2, j3))
            assert len(triples) == h * (h - 1) * (h - 2) or h == 20
            if h == 3:
                assert triples == {(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)}
                counts = np.array([np.sum((j1 == t[0]) & (j2 == t[1])) for t in sorted(triples)])
                assert np.all(np.abs(counts / 20000.0 - 1.0 / 6.0) < 0.01)  # uniform
        else:
            assert np.all(j3 == 0)
    # the draws at the edges: d = 0 and the largest double below 1
    top = np.nextafter(1.0, 0.0)
    for h in (2, 3, 5):
        for a in (0.0, top):
            for b in (0.0, top):
                for c in (0.0, top):
                    j1, j2, j3 = oracle.partners(np.array([a]), np.array([b]), np.array([c]), h, h >= 3)
                    assert len({int(j1[0]), int(j2[0])} | ({int(j3[0])} if h >= 3 else set())) == (3 if h >= 3 else 2)
                    assert max(j1[0], j2[0], j3[0]) < h


def test_row_sum_is_the_butterfly_of_the_lanes():
    rs = np.random.RandomState(3)
    for n, lpr in ((1, 16), (5, 16), (16, 16), (17, 16), (64, 16), (65, 32), (96, 32), (129, 64), (200, 64)):
        T = rs.standard_normal((7, n)) * 10.0 ** rs.randint(-3, 4, (7, n))
        lanes = np.zeros((7, lpr))
        for e in range(n):
            lanes[:, e % lpr] = lanes[:, e % lpr] + T[:, e]
        while lanes.shape[1] > 1:  # v += v[lane ^ 1] leaves pairs of equal sums; then ^ 2 ...: a tree over neighbours
            lanes = lanes[:, 0::2] + lanes[:, 1::2]
        assert np.array_equal(oracle.row_sum(T), lanes[:, 0]), n
        assert np.allclose(oracle.row_sum(T), T.sum(axis=1), rtol=1e-12, atol=1e-9)


def test_burn_and_thin_select_rows_of_the_unthinned_run():
    bounds = [[-5.12, 5.12]] * 2
    o = {"chains": 3, "walkers": 6, "maxiter": 30, "seed": 2, "moves": cases.MIXTURE}
    full = oracle.sample("rastrigin", bounds, options=dict(o))
    for burn, thin, rows in ((7, 3, 8), (29, 1, 1), (5, 26, 1), (0, 2, 15), (0, 1, 30), (10, 1, 20)):
        told = []
        cut = oracle.sample("rastrigin", bounds, options=dict(o, burn=burn, thin=thin),
                            callback=lambda xk, state: told.append((state.nit, state.xall.shape[1])))
        recorded = np.arange(burn, 30, thin)
        assert cut.xall.shape == (3, rows, 6, 2) and cut.funall.shape == (3, rows, 6) and len(recorded) == rows
        assert np.array_equal(cut.xall, full.xall[:, recorded]) and np.array_equal(cut.funall, full.funall[:, recorded])
        for key in ("x", "fun", "accept_ratio", "accept_ratios", "nacc"):  # over all samples
            assert np.array_equal(cut[key], full[key]), key
        assert (cut.burn, cut.thin) == (burn, thin)
        # the callback comes once per sample; its xall holds the recorded rows among the samples before the newest
        assert told == [(i + 1, int(np.sum(recorded < max(i, 1)))) for i in range(30)]


# ---- the moves sample correctly ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def gauss_run(name, seed):
    x0, o = cases.gauss_options(name, seed)
    return oracle.sample(cases.rotated_value, cases.GAUSS_BOUNDS, x0=x0, options=o)


@functools.lru_cache(maxsize=None)
def bimodal_run(name, seed):
    return oracle.sample(cases.bimodal_value, cases.BIMODAL_BOUNDS,
                         options=cases.bimodal_options(cases.BIMODAL_MOVES.get(name), seed))


@pytest.mark.parametrize("seed", cases.TEST_SEEDS)
@pytest.mark.parametrize("name", list(cases.GAUSS_RUNS))
def test_each_move_samples_the_rotated_gaussian(name, seed):
    """The per-axis variance over sigma^2 in the rotated frame within 3 x the largest deviation of five seeds
    (profiles/sample_ensemble_moves_cases.txt, tools/sample_ensemble_moves_cases.py)."""
    res = gauss_run(name, seed)
    r = cases.variance_ratio(res.xall, cases.GAUSS_RUNS[name][2])
    print(name, "seed", seed, "variance / sigma^2", r.min(), "..", r.max(), "accept_ratio", res.accept_ratio, "bound",
          cases.GAUSS_BOUND[name])
    assert cases.GAUSS_BOUND == {"de": 3.0 * 0.0136, "snooker": 3.0 * 0.0256, "mixture": 3.0 * 0.0226}
    assert np.all(np.abs(r - 1.0) <= cases.GAUSS_BOUND[name])
    assert 0.05 < res.accept_ratio < 0.6


@pytest.mark.parametrize("seed", cases.TEST_SEEDS)
@pytest.mark.parametrize("name", list(cases.BIMODAL_MOVES))
def test_the_de_move_finds_the_weights_of_two_separated_modes(name, seed):
    """The pooled share of the kept samples in the heavy mode within 3 x the largest deviation of five seeds from 0.75."""
    res = bimodal_run(name, seed)
    share, each = cases.heavy_share(res.xall)
    print(name, "seed", seed, "share", share, "per ensemble", each.min(), "..", each.max(), "accept_ratio", res.accept_ratio,
          "bound", cases.BIMODAL_BOUND[name])
    assert cases.BIMODAL_BOUND == {"de": 3.0 * 0.0081, "de+snooker": 3.0 * 0.0245}
    assert abs(share - cases.BIMODAL_SHARE) <= cases.BIMODAL_BOUND[name]
    if name == "de":  # no ensemble sits in one mode (with the snooker move one in a hundred does: _ensemble_moves_cases.py)
        assert 0.5 < each.min() and each.max() < 0.95


@pytest.mark.parametrize("seed", cases.TEST_SEEDS)
def test_the_stretch_move_alone_keeps_the_split_of_its_start(seed):
    """The condition that the target discriminates: stretch misses 0.75 by more than 0.15, its ensembles frozen."""
    res = bimodal_run("stretch", seed)
    share, each = cases.heavy_share(res.xall)
    print("stretch seed", seed, "share", share, "per ensemble", each.min(), "..", each.max())
    assert abs(share - cases.BIMODAL_SHARE) > cases.STRETCH_MISSES_BY == 0.15
    assert each.min() == 0.0 and each.max() > 0.9 and "moves" not in res
