"""GPU: the kernels of method="smc" (csrc/sx_sample_smc.hip) ONE CALL AT A TIME through the C ABI, on inputs the host writes
(tests/_smc_kernel_cases.py), against tests/_smc_oracle.py's stage_once / gather_once / mutate_once:

1. sx_smc_stage on planted values, records and acceptance counts at every particle count on both sides of K = 1 | 2 | 3,
   with NaN / +inf on the edges of a thread, a wave and the population, mid-run, at maxiter, closing, stale and dead;
2. sx_smc_resample on planted particles and ancestors (outside [0, P) too), every axis with its own box, between guard rows;
3. sx_smc_mutate from planted particles, frozen and live populations inside one workgroup;
4. sx_smc_propose / sx_smc_decide around a caller's objective in every row form, bit for bit the resident run, and the contract
   of a frozen population: the caller's objective is only ever given points of the box.

Tolerances are the project's (tests/test_gpu_sample_smc.py): ancestors, counts and the integers of a record exact, beta, log Z,
ESS, scale, step and values 1e-6 relative, samples 1e-6 of the axis' width; what a kernel only moves is compared bit for bit.
Every case was admitted by the restatement alone (tests/test_sample_smc_kernels_host.py).  Nothing here can fault: every index
a wrong kernel could form stays inside an allocation, every shape is one the entry points accept."""
import ctypes as C
import os
import sys
import time
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _smc_kernel_cases as kc  # noqa: E402
import _smc_oracle as oracle  # noqa: E402
from test_gpu_sample_batched import device_objective  # noqa: E402
from test_gpu_sample_smc import KEYS, check_result, close_values, run  # noqa: E402

pytestmark = pytest.mark.gpu

ST = oracle
CANARY, CANARY_INT = -1.2345e300, -12345
WORST = {}  # part -> name -> the largest relative deviation seen
SPENT = {}  # part -> seconds


@pytest.fixture(scope="module")
def sa():
    import stochopy_amd

    yield stochopy_amd
    print("\n    the largest relative deviations from the restatement, and the time of each part")
    for part in sorted(SPENT):
        worst = "  ".join("%s %.3g" % kv for kv in sorted(WORST.get(part, {}).items()))
        print("    part %-8s %6.2f s   %s" % (part, SPENT[part], worst))


def deviation(part, name, got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    with np.errstate(all="ignore"):
        d = np.abs(got - want) / np.abs(want)
    d = float(np.max(np.where(np.isfinite(d), d, 0.0), initial=0.0))
    WORST.setdefault(part, {})[name] = max(WORST.get(part, {}).get(name, 0.0), d)
    return d


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype.itemsize == 8 else np.uint32)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


class Device:
    """The arrays of one sx_smc_args, each between guards that must come back unchanged, and the entry points on them."""
    SHAPES = {"x0": "Rn", "x1": "Rn", "f0": "R", "f1": "R", "anc": "R", "nacc": "R", "step": "Cn", "state": "C8"}

    def __init__(self, sa, Cn, P, n, lower, upper, fun=None, maxiter=100, ess=0.5, target=0.234, scale=0.9):
        import torch

        from stochopy_amd import _device, _lib
        from stochopy_amd.sample import _smc

        self.torch, self.L, self.check = torch, _lib.lib(), _lib.check
        self.ctx = _device.Context()
        s = types.SimpleNamespace(chains=Cn, particles=P, ndim=n, lower=np.ascontiguousarray(lower, dtype=np.float64),
                                  upper=np.ascontiguousarray(upper, dtype=np.float64), fun_id=_lib.FUN_IDS[fun] if fun else 0,
                                  steps=kc.M, maxiter=maxiter, ess=ess, target=target, scale=scale, key=kc.KEY)
        with torch.cuda.stream(self.ctx.stream):
            self.dev, self.a = _smc.smc_args(self.ctx, s)
            sizes = {"Rn": Cn * P * n, "R": Cn * P, "Cn": Cn * n, "C8": Cn * ST.ST_WORDS}
            self.guard = max(64, kc.GUARD_ROWS * n)
            self.whole = {}
            for name, kind in self.SHAPES.items():
                dtype = self.dev[name].dtype
                canary = CANARY if dtype == torch.float64 else CANARY_INT
                self.whole[name] = torch.full((sizes[kind] + 2 * self.guard,), canary, dtype=dtype, device=self.ctx.device)
                self.dev[name] = self.whole[name][self.guard:self.guard + sizes[kind]]
                self.dev[name].zero_()
            a = self.a
            a.x[0], a.x[1], a.f[0], a.f[1] = (self.dev[k].data_ptr() for k in ("x0", "x1", "f0", "f1"))
            for name in ("anc", "nacc", "step", "state"):
                setattr(a, name, _device.ptr(self.dev[name]))

    def put(self, name, values):
        t = self.torch
        with t.cuda.stream(self.ctx.stream):
            if np.ndim(values) == 0:  # (a filled host array: a NaN keeps its payload on the way)
                values = np.full(self.dev[name].numel(), values, dtype={"anc": np.int32, "nacc": np.int64}.get(name, np.float64))
            self.dev[name].copy_(t.from_numpy(np.ascontiguousarray(values).reshape(-1)))

    def get(self, name):
        with self.torch.cuda.stream(self.ctx.stream):
            return self.dev[name].cpu().numpy()

    def raw(self, name, *args):
        with self.torch.cuda.stream(self.ctx.stream):
            return getattr(self.L, name)(C.byref(self.a), *args, self.ctx.stream_ptr)

    def call(self, name, *args):
        self.check(self.raw(name, *args), name)

    def guards_are_whole(self):
        g = self.guard
        for name, whole in self.whole.items():
            with self.torch.cuda.stream(self.ctx.stream):
                host = whole.cpu().numpy()
            canary = CANARY if host.dtype == np.float64 else CANARY_INT
            assert np.all(host[:g] == canary) and np.all(host[-g:] == canary), name
        return True


def timed(part, t0):
    SPENT[part] = SPENT.get(part, 0.0) + time.time() - t0


# ---- 1. the stage kernel on planted values -------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", kc.STAGE_CASES, ids=kc.stage_id)
def test_one_stage_call_on_planted_values(sa, case):
    t0 = time.time()
    _, inp, (want, want_anc) = kc.stage_admitted(case)
    P, s, before = case.P, inp["s"], inp["record"]
    assert P <= sa.sample._smc.max_particles() and oracle.MAX_PARTICLES == sa.sample._smc.max_particles()
    d = Device(sa, kc.C, P, 1, [0.0], [1.0], maxiter=case.maxiter, ess=case.ess, target=case.target)
    src, other = ("f0", "f1") if (s - 1) % 2 == 0 else ("f1", "f0")
    d.put(src, inp["F"]), d.put(other, kc.NAN_SENTINEL), d.put("state", before), d.put("nacc", inp["nacc"])
    d.put("anc", kc.SENTINEL)
    d.call("sx_smc_stage", s)
    rec, anc = d.get("state").reshape(kc.C, ST.ST_WORDS), d.get("anc").reshape(kc.C, P)
    took = want[:, ST.ST_STAGES] == s
    devs = [deviation("1 stage", name, rec[took, word], want[took, word])
            for name, word in (("beta", ST.ST_BETA), ("logZ", ST.ST_LOGZ), ("ess", ST.ST_ESS), ("scale", ST.ST_SCALE))]
    print("    %-26s status %s  deviations: beta %.2e logZ %.2e ess %.2e scale %.2e" % (kc.stage_id(case), rec[:, 0], *devs))
    # the ancestors: exact where the population took part, left alone elsewhere
    assert np.array_equal(anc[took], want_anc[took]) and np.all(anc[~took] == kc.SENTINEL)
    # the record: integers, r and the count exact; what the stage did not touch bit for bit
    for word in (ST.ST_STATUS, ST.ST_STAGES, ST.ST_COUNT, ST.ST_ACCEPT):
        assert np.array_equal(rec[:, word], want[:, word]), word
    for word in (ST.ST_BETA, ST.ST_LOGZ, ST.ST_ESS, ST.ST_SCALE):
        assert close_values(rec[took, word], want[took, word]), word
        assert same_bits(rec[~took, word], np.where(np.isneginf(want[~took, word]), -np.inf, before[~took, word])), word
    if case.start == "stale":
        assert same_bits(rec, before)
    if case.start == "closing":
        assert same_bits(rec[:, [0, 1, 2, 3, 4, 6]], before[:, [0, 1, 2, 3, 4, 6]]) and not took.any()
    if case.dead:
        m = kc.MIDDLE
        assert rec[m, ST.ST_STATUS] == -2.0 and rec[m, ST.ST_LOGZ] == -np.inf and rec[m, ST.ST_BETA] == before[m, ST.ST_BETA]
        assert not took[m] and took[[0, 2]].all()
    # whatever the restatement says
    for c in np.flatnonzero(took):
        assert kc.resampling_is_sound(inp["F"][c], before[c, ST.ST_BETA], rec[c, ST.ST_BETA], anc[c])
    if case.profile == "a" and case.start == "fresh":
        m = kc.MIDDLE
        assert rec[m, ST.ST_BETA] == 1.0 and rec[m, ST.ST_ESS] == 1.0 and rec[m, ST.ST_LOGZ] == -2.5
    if case.profile == "e":
        assert np.all(anc[kc.MIDDLE] == P - 1) and rec[kc.MIDDLE, ST.ST_BETA] == 2.0 ** -52
    # the call reads its values and counts, and writes the records and anc alone
    assert same_bits(d.get(src).reshape(kc.C, P), inp["F"]) and np.array_equal(d.get("nacc").reshape(kc.C, P), inp["nacc"])
    assert same_bits(d.get(other), np.full(kc.C * P, kc.NAN_SENTINEL)) and d.guards_are_whole()
    timed("1 stage", t0)


def test_the_stage_entry_points_refuse_before_they_launch(sa):
    d = Device(sa, kc.C, 4, 1, [0.0], [1.0], maxiter=5)
    d.put("anc", kc.SENTINEL)
    assert d.raw("sx_smc_stage", 0) == -1 and d.raw("sx_smc_stage", 7) == -1 and d.raw("sx_smc_stage", -1) == -1
    assert d.raw("sx_smc_resample", 0) == -1 and d.raw("sx_smc_resample", 6) == -1
    assert d.raw("sx_smc_mutate", 0) == -1 and d.raw("sx_smc_mutate", 6) == -1
    for field, bad in (("P", 3), ("P", oracle.MAX_PARTICLES + 1), ("ess", 0.0), ("ess", 1.0), ("target", 1.0), ("C", 0)):
        good = getattr(d.a, field)
        setattr(d.a, field, bad)
        assert d.raw("sx_smc_stage", 1) == -1, field
        setattr(d.a, field, good)
    assert np.all(d.get("anc") == kc.SENTINEL) and not d.get("state").any() and d.guards_are_whole()


# ---- 2. the gather kernel on planted state -------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", kc.GATHER_P)
@pytest.mark.parametrize("n", kc.GATHER_N)
def test_one_gather_call_on_planted_state(sa, n, P):
    from stochopy_amd import _lib

    t0 = time.time()
    assert kc.WIDE_FROM == _lib.wide_from()
    lower, upper = kc.box(n)
    d = Device(sa, kc.C, P, n, lower, upper)
    worst = 0.0
    for s in (1, 2):  # both buffer directions
        src, dst = ("0", "1") if s == 1 else ("1", "0")
        for kind, skip in kc.GATHER_ANCS:
            x, f, anc, record = kc.gather_inputs(n, P, s, kind)
            d.put("x" + src, x), d.put("f" + src, f), d.put("anc", anc), d.put("state", record)
            d.put("x" + dst, kc.NAN_SENTINEL), d.put("f" + dst, kc.NAN_SENTINEL), d.put("step", kc.NAN_SENTINEL)
            d.call("sx_smc_resample", s)
            gx, gf = d.get("x" + dst).reshape(kc.C, P, n), d.get("f" + dst).reshape(kc.C, P)
            step = d.get("step").reshape(kc.C, n)
            wx, wf, wstep = oracle.gather_once(x, f, anc, record[:, ST.ST_SCALE], lower, upper)
            took = np.array([c != skip for c in range(kc.C)])
            # a pure move: bit for bit, rows outside [0, P) held at 0 and P - 1
            assert same_bits(gx[took], wx[took]) and same_bits(gf[took], wf[took]), (s, kind)
            assert close_values(step[took], wstep[took]), (s, kind)
            worst = max(worst, deviation("2 gather", "step", step[took], wstep[took]))
            if kind == "one":  # the floor of a collapsed axis, each axis its own half-width
                floor = np.array(kc.GATHER_SCALE)[:, None] * 1.0e-8 * (0.5 * (upper - lower))
                assert close_values(step, floor), (s, kind)
            if kind == "outside":
                m = kc.MIDDLE
                assert same_bits(gx[m, [0, 1, P - 2, P - 1]], x[m, [0, 0, P - 1, P - 1]])
            # a population whose record names another stage keeps what it held
            assert same_bits(gx[~took], np.full_like(gx[~took], kc.NAN_SENTINEL)), (s, kind)
            assert same_bits(gf[~took], np.full_like(gf[~took], kc.NAN_SENTINEL)), (s, kind)
            assert same_bits(step[~took], np.full_like(step[~took], kc.NAN_SENTINEL)), (s, kind)
            # the call writes nothing else
            assert same_bits(d.get("x" + src).reshape(x.shape), x) and same_bits(d.get("f" + src).reshape(f.shape), f)
            assert same_bits(d.get("state").reshape(record.shape), record) and np.array_equal(d.get("anc").reshape(anc.shape), anc)
    assert d.guards_are_whole()
    print("    gather n=%-4d P=%-3d the largest deviation of a step %.2e" % (n, P, worst))
    timed("2 gather", t0)


# ---- 3. the mutation kernel from planted particles -----------------------------------------------------------------------------
@pytest.mark.parametrize("case", kc.MUTATE_CASES, ids=kc.mutate_id)
def test_one_mutation_call_from_planted_particles(sa, case):
    t0 = time.time()
    _, inp, (wx, wf, wnacc), shares = kc.mutate_admitted(case)
    fun, n = case
    Cn, P, s = kc.MUTATE_C, kc.MUTATE_P, kc.MUTATE_S
    d = Device(sa, Cn, P, n, inp["lower"], inp["upper"], fun=fun)
    d.put("x1", inp["x"]), d.put("f1", inp["f"]), d.put("step", inp["step"]), d.put("state", inp["record"])
    d.put("x0", kc.NAN_SENTINEL), d.put("f0", kc.NAN_SENTINEL), d.put("nacc", -3), d.put("anc", kc.SENTINEL)
    d.call("sx_smc_mutate", s)
    x, f, nacc = d.get("x1").reshape(Cn, P, n), d.get("f1").reshape(Cn, P), d.get("nacc").reshape(Cn, P)
    live, frozen = inp["live"], ~inp["live"]
    width = inp["upper"] - inp["lower"]
    dx = float(np.max(np.abs(x[live] - wx[live]) / width))
    df = deviation("3 mutate", "f", f[live], wf[live])
    WORST["3 mutate"]["x/width"] = max(WORST["3 mutate"].get("x/width", 0.0), dx)
    print("    %-22s outside %.2f accepted %d rejected %d  deviations: x / width %.2e f %.2e" % (kc.mutate_id(case), *shares, dx, df))
    assert np.array_equal(nacc[live], wnacc[live])
    assert np.all(np.abs(x[live] - wx[live]) <= 1e-6 * width) and close_values(f[live], wf[live])
    # frozen populations run along in the same workgroups and store nothing
    assert same_bits(x[frozen], inp["x"][frozen]) and same_bits(f[frozen], inp["f"][frozen]) and np.all(nacc[frozen] == -3)
    # the call writes the particles, their values and nacc alone
    assert same_bits(d.get("x0"), np.full(Cn * P * n, kc.NAN_SENTINEL)) and same_bits(d.get("f0"), np.full(Cn * P, kc.NAN_SENTINEL))
    assert same_bits(d.get("state").reshape(Cn, ST.ST_WORDS), inp["record"]) and same_bits(d.get("step").reshape(Cn, n), inp["step"])
    assert np.all(d.get("anc") == kc.SENTINEL) and d.guards_are_whole()
    timed("3 mutate", t0)


# ---- 4. the propose / decide pair at every row form, and the frozen contract ---------------------------------------------------
@pytest.mark.parametrize("fun", kc.PAIR_FUNS)
@pytest.mark.parametrize("n", kc.PAIR_N)
def test_a_callers_objective_is_the_resident_run_in_every_row_form(sa, n, fun):
    from stochopy_amd import _lib

    t0 = time.time()
    assert kc.WIDE_FROM == _lib.wide_from()
    opts = dict(kc.PAIR_LONGEST if n == kc.WIDE_FROM else kc.PAIR_OPTIONS, seed=7 + n)
    bounds = [[-kc.PAIR_BOUND, kc.PAIR_BOUND]] * n
    resident = run(sa, getattr(sa.factory, fun), bounds, **opts)
    got = run(sa, device_objective(sa, fun), bounds, **opts)
    assert np.all(np.isfinite(resident.funall)) and resident.nit >= 2  # (equality means something)
    for key in KEYS:
        assert np.array_equal(resident[key], got[key]), key
    assert got.nfev == resident.nfev and got.accept_ratio == resident.accept_ratio and got.accept_ratio > 0.0
    timed("4 pair", t0)


def test_a_frozen_population_proposes_its_own_particles(sa):
    """Populations that end after stages 1, 8, 0 (status -2) and 2 in a box that excludes the origin: at every step of every
    later stage the caller's objective is given the ended population's own final particles, bit for bit, and never a point
    outside the box.  (Before smc_propose_kernel read a frozen particle from the buffer its own record names, it read
    x[s & 1]: population 2 gave the objective the rows of the never-written buffer 1 at every odd stage -- 64 rows of zeros --
    and populations 0 and 3 their rows from before the last resampling at every second stage.)  The box is asserted for the
    draw and for ended populations: a live particle's proposal outside the box is evaluated and its value dropped, by design."""
    import torch

    t0 = time.time()
    seed, P, M = kc.FROZEN_GPU_SEED, kc.FROZEN_P, kc.FROZEN_OPTIONS["steps"]
    seen = []

    def fun(X):
        seen.append(X.clone())
        return kc.frozen_values(X)

    fun.__name__ = "mixed"
    got = run(sa, sa.factory.batched(fun), kc.FROZEN_BOUNDS, seed=seed, **kc.FROZEN_OPTIONS)
    torch.cuda.synchronize()
    want = oracle.sample(kc.frozen_values, kc.FROZEN_BOUNDS, dict(kc.FROZEN_OPTIONS, seed=seed))
    assert tuple(got.stages) == kc.FROZEN_STAGES and tuple(got.statuses) == kc.FROZEN_STATUSES
    assert len(seen) == 1 + M * got.nit
    seen = [X.cpu().numpy().reshape(4, P, kc.FROZEN_NDIM) for X in seen]
    lower, upper = np.transpose(kc.FROZEN_BOUNDS)
    outside = [(k, c) for k, X in enumerate(seen) for c in range(4) if not np.all((X[c] >= lower) & (X[c] <= upper))
               and (k == 0 or (k - 1) // M + 1 > got.stages[c])]
    print("    calls of the objective in which an ended population's rows lie outside the box (call, population):", outside)
    strangers = []
    for c, s0 in enumerate(kc.FROZEN_STAGES):
        for s in range(s0 + 1, got.nit + 1):
            for m in range(1, M + 1):
                if not same_bits(seen[1 + (s - 1) * M + (m - 1)][c], got.xall[c]):
                    strangers.append((c, s, m))
    print("    (population, stage, step) at which an ended population did not propose its own particles:", strangers)
    assert np.all((seen[0] >= lower) & (seen[0] <= upper))  # stage 0: the draw
    assert not outside and not strangers
    check_result(got, want, float(np.max(upper - lower)))
    timed("4 pair", t0)
