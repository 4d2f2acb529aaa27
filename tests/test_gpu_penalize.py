"""constraints="Penalize" on the device, one call at a time (sx_cma_penalize = cma_penalize_launch, csrc/sx_cma_loop.hip:
cma_rank_kernel -> cma_penalty_kernel -> sx_cmaes_eval_penalized -> cma_add_penalty_kernel; cmaes/_constraints.py:4-82), and
sx_cmaes_eval_penalized on the narrow rows (eval_kernel with clip / pen_v / pen_out, 16 / 32 / 64 lanes per row).

Bookkeeping: every planted state of tests/_penalize_abi.py (checked on the CPU by tests/test_penalize_host.py) is uploaded,
the entry is called once and the whole workspace read back.  The reference is oracle.engine.PenalizeState.apply restated in
np.longdouble, the quartiles np.percentile's own.  Exact: count, valid, ini, pen_order, the set of grown coordinates, every
history slot but the new entry, every weight that was neither filled nor grown, the spare slot.  Bounds, u = 2^-53:
  new history entry   (n + 6) u     the diagonal's sum of n positive terms in any order (n - 1), q75 - q25, / n, sd / n, /,
                                    sigma sigma, / (6), one for the second-order terms
  filled weight       (n + 8) u     the entry above may be the median or one of its two halves; their mean, x 2.0002
  grown weight        (n + 8) u + FAC_BOUND    x the growth factor 1.2^min(1, mueff / 10 n): the device's pow and the product
  v                   V_BOUND       w / exp(0.9 (log dc - mean log dc)): the device's log and exp, and a sum of logarithms of
                                    either sign, whose error no formula in n alone bounds
  pen                 (n + 4) u     c - x, its square, x v, a sum of n non-negative terms in any order
FAC_BOUND and V_BOUND are measured, not derived: 4 x the largest relative deviation from the long-double restatement seen
over all cases on an MI355X (profiles/penalize_gpu_tests.txt): growth factor 1.695e-16 -> FAC_BOUND = 6.8e-16;
v 2.282e-15 -> V_BOUND = 9.2e-15 (both rounded up).  Every test prints its deviations before it asserts.
The final fit is the objective of the clipped rows (the device's own value, from a call of sx_cmaes_eval_penalized without
weights) + the device's pen, to the bit: one rounding.

Evaluation: all seven objectives at every lanes-per-row class and on each side of its batch sizes, up to the last narrow row;
pen against the long-double sum, the objective within the bounds of tests/_objective_exact.py (as
tests/test_gpu_objective_domains.py applies them) on the clipped, un-standardised rows; a NaN element stays NaN (the
reference's np.where keeps it), an infinite one is clipped, and an infinite excess times a zero weight is NaN as in numpy."""
import numpy as np
import pytest

import _objective_exact as ox
import _penalize_abi as pa
import oracle
from oracle.objectives import OBJECTIVES

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not ox.have_longdouble(),
                                 reason="np.longdouble has fewer than 63 mantissa bits here: no reference finer than double")]

LD = np.longdouble
U = pa.U
FAC_BOUND = 6.8e-16
V_BOUND = 9.2e-15
SEEN = {"fac": 0.0, "v": 0.0}


@pytest.fixture(scope="module")
def sa():
    import stochopy_amd

    return stochopy_amd


@pytest.fixture(scope="module")
def ctx(sa):
    from stochopy_amd import _device

    return _device.Context()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def rel(got, ref):
    """max |got - ref| / |ref| against a long-double reference (0 for an empty selection)."""
    ref, got = np.atleast_1d(np.asarray(ref, dtype=LD)), np.atleast_1d(np.asarray(got, dtype=np.float64))
    assert np.all(got[ref == 0] == 0.0)  # (a weight of 0 stays 0, and so does its v)
    ref, got = ref[ref != 0], got[ref != 0]
    if ref.size == 0:
        return 0.0
    return float(np.max(np.abs(got.astype(LD) - ref) / np.abs(ref)))


def clip_keep_nan(X):
    return np.where(X < -1.0, -1.0, np.where(X > 1.0, 1.0, X))  # cmaes/_constraints.py:29-31


def penalty_exact(X, v):
    x = X.astype(LD)
    with np.errstate(invalid="ignore"):
        c = np.where(x < -1, LD(-1), np.where(x > 1, LD(1), x))
        return ((c - x) ** 2 * v.astype(LD)).sum(axis=1)


def check_penalty(got, ref, n, what):
    """pen within (n + 4) u of the long-double sum; an exact zero, a NaN and an infinity are themselves."""
    fin = np.isfinite(ref)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), what
    assert np.array_equal(got[~fin & ~np.isnan(ref)], ref[~fin & ~np.isnan(ref)].astype(np.float64)), what
    zero = fin & (ref == 0)
    assert np.array_equal(bits(got[zero]), bits(np.zeros(int(zero.sum())))), what
    pos = fin & (ref != 0)
    dev = rel(got[pos], ref[pos])
    assert dev <= (n + 4) * U, (what, dev, (n + 4) * U)
    return dev


def check_objective(name, Xu, got, what):
    """The objective of the un-standardised rows Xu (double): NaN where a row holds one; elsewhere within the measured bound
    of tests/_objective_exact.py, and numpy's bits for the objectives of + - * only."""
    with np.errstate(all="ignore"):
        bad = np.isnan(OBJECTIVES[name](Xu))  # (every row that holds a NaN -- but rosenbrock of one element has no term)
    assert np.array_equal(bad, np.isnan(Xu).any(axis=1) & (name != "rosenbrock" or Xu.shape[1] > 1)), what
    assert np.isnan(got[bad]).all() and np.isfinite(got[~bad]).all(), what
    if bad.all():
        return 0.0
    E, ratio, ref = ox.measure(name, Xu[~bad], got[~bad])
    assert ratio.max() <= 1.0, (what, float(ratio.max()), E)
    if name in ox.BIT_EQUAL:
        assert np.array_equal(got[~bad], OBJECTIVES[name](Xu[~bad])), what
    if name in ("quartic", "styblinski_tang"):
        assert np.array_equal(got[~bad], ox.kernel_association(name, Xu[~bad])), what
    return float(ratio.max())


# ---- 2. the bookkeeping, one call at a time ----------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", pa.tags())
def test_bookkeeping_one_call(ctx, tag):
    case = pa.cases()[tag]
    n, P = case.n, case.P
    dev = pa.run(ctx, case)
    assert dev.rc == 0, dev.message
    got, r = pa.unpack_ws(dev.ws, n, P), pa.restate(case, LD)
    # the flags, the ranking, the untouched slots
    assert (got["count"], got["valid"], got["ini"], got["spare"]) == (r.count, r.valid, r.ini, -3.0)
    assert np.array_equal(dev.order, np.argsort(case.fit, kind="stable"))
    assert np.array_equal(bits(dev.state), bits(dev.state_before))
    want = pa.unpack_ws(dev.ws_before, n, P)["hist"]
    want[:r.count - 1] = np.array(r.hist[:-1], dtype=np.float64)  # (old entries are doubles: pushed behind, or shifted in order)
    keep = np.arange(pa.HIST) != r.count - 1
    assert np.array_equal(bits(got["hist"][keep]), bits(want[keep])), np.flatnonzero(bits(got["hist"]) != bits(want))
    # the new entry
    new = got["hist"][r.count - 1]
    if r.fresh:
        hist_dev = rel(new, r.delta)
        assert hist_dev <= (n + 6) * U, (hist_dev, (n + 6) * U)
    else:
        hist_dev = 0.0
        assert bits(new) == bits(np.float64(r.delta))
    # the weights: grown coordinates are the ones beyond the midpoint between a weight and its grown value
    base = np.full(n, r.fill, dtype=LD) if r.filled else case.w.astype(LD)
    grown = got["w"].astype(LD) > base * (1 + (r.fac - 1) / 2)
    assert np.array_equal(grown, r.grown), (np.flatnonzero(grown), np.flatnonzero(r.grown))
    rest = ~r.grown
    if r.filled:
        assert len(set(bits(got["w"][rest]).tolist())) <= 1  # one fill value
        fill_dev = rel(got["w"][rest], r.w[rest])
        assert fill_dev <= (n + 8) * U, (fill_dev, (n + 8) * U)
        dev_base = np.full(n, got["w"][rest][0] if rest.any() else np.float64(r.fill))
    else:
        fill_dev = 0.0
        assert np.array_equal(bits(got["w"][rest]), bits(case.w[rest]))
        dev_base = case.w
    fac_dev = rel(got["w"][r.grown], dev_base[r.grown].astype(LD) * r.fac)  # the factor alone: against the device's own base
    grown_dev = rel(got["w"][r.grown], r.w[r.grown])
    v_dev = rel(got["v"], r.v)
    SEEN["fac"], SEEN["v"] = max(SEEN["fac"], fac_dev), max(SEEN["v"], v_dev)
    pen_ref = penalty_exact(case.arx, got["v"])
    print("penalize_bookkeeping %-28s n=%-4d P=%-2d grown=%-3d hist=%.2e fill=%.2e fac=%.3e v=%.3e"
          % (tag, n, P, int(r.grown.sum()), hist_dev, fill_dev, fac_dev, v_dev))
    assert np.isfinite(got["v"]).all() and np.isfinite(got["pen"]).all()
    assert grown_dev <= (n + 8) * U + FAC_BOUND, (grown_dev, fac_dev)
    assert fac_dev <= ((n + 8) * U if r.filled and not rest.any() else 0.0) + FAC_BOUND, fac_dev
    assert v_dev <= V_BOUND, v_dev
    # the penalty pass and the final fitness
    check_penalty(got["pen"], pen_ref, n, tag)
    Xu = clip_keep_nan(case.arx) * case.xstd + case.xm
    check_objective(case.fun, Xu, dev.f_raw, tag)
    assert np.array_equal(bits(dev.fit), bits(dev.f_raw + got["pen"]))


def test_measured_deviations_stay_inside_their_bounds():
    """What the cases above measured (this run), against the constants in the docstring."""
    print("penalize_measured growth factor max %.3e (bound %.3e)   v max %.3e (bound %.3e)"
          % (SEEN["fac"], FAC_BOUND, SEEN["v"], V_BOUND))
    assert SEEN["fac"] <= FAC_BOUND + (1 + 8) * U and SEEN["v"] <= V_BOUND  # (n = 1, filled: no untouched weight to divide by)


@pytest.mark.parametrize("form", pa.FORMS)
def test_bookkeeping_rests_once_the_run_is_done(ctx, form):
    """state.done: no ranking, no bookkeeping, no penalty added -- weights, v, history and flags stay as they are.  (The
    evaluation between them has no state to look at: it still leaves the objective of the clipped rows in fit, which
    nothing reads after the stop.)"""
    case = pa.cases()["shape-%s-n65-P8" % form]
    dev = pa.run(ctx, case, done=1)
    assert dev.rc == 0
    got, was = pa.unpack_ws(dev.ws, case.n, case.P), pa.unpack_ws(dev.ws_before, case.n, case.P)
    for k in ("w", "v", "hist", "count", "valid", "ini", "spare"):
        assert np.array_equal(bits(got[k]), bits(was[k])), k
    assert np.all(dev.order == -1)
    assert np.array_equal(bits(dev.fit), bits(dev.f_raw))  # (no penalty added)


@pytest.mark.parametrize("form", pa.FORMS)
def test_guard_rejects_a_history_beyond_its_slots(ctx, form):
    """n = 472, P = 6: 20 + 3 n / P + 1 = 257 entries: the entry says so and launches nothing."""
    case = pa.make("guard-" + form, form, 472, 6, gen=3, count=7, valid=1, ini=1, outside=(0, 471))
    assert not pa.admitted(case.n, case.P) and pa.admitted(470, 6)
    dev = pa.run(ctx, case)
    assert dev.rc != 0 and "spread history of at most 256 entries" in dev.message
    assert np.array_equal(bits(dev.ws), bits(dev.ws_before)) and np.array_equal(bits(dev.fit), bits(case.fit))
    assert np.all(dev.order == -1)


@pytest.mark.parametrize("n,device_loop", [(470, True), (472, False)])
def test_guard_in_the_public_call(sa, n, device_loop, monkeypatch):
    """minimize(method="vdcma", constraints="Penalize") at P = 6: the device-resident loop at n = 470, the host-driven one
    at n = 472 (optimize/_evolution.py device_loop_serves); both follow the oracle."""
    from stochopy_amd.optimize import _vdcma

    taken = []
    orig = _vdcma._VdDeviceRun.__init__

    def spy(self, *a, **k):
        taken.append(k.get("penalize"))
        orig(self, *a, **k)

    monkeypatch.setattr(_vdcma._VdDeviceRun, "__init__", spy)
    lo, hi = 0.5, 3.0
    bounds = [[lo, hi]] * n
    opts = {"maxiter": 5, "popsize": 6, "seed": 77, "sigma": 0.25, "constraints": "Penalize", "return_all": True,
            "verbosity": 1.0, "ftol": -1.0, "xtol": 0.0}
    ref = oracle.minimize("sphere", bounds, method="vdcma", options=dict(opts), rng="philox")
    got = sa.optimize.minimize(sa.factory.sphere, bounds, method="vdcma", options=dict(opts, backend="hip", rng="philox"))
    assert taken == ([True] if device_loop else [])
    assert (got.nit, got.nfev, got.status) == (ref.nit, ref.nfev, ref.status) and ref.nit == 5
    assert np.allclose(got.funall, ref.funall, rtol=1e-6, atol=1e-300), np.abs(got.funall / ref.funall - 1).max()
    assert np.allclose(got.xall, ref.xall, rtol=1e-5, atol=1e-6 * (hi - lo))
    assert np.isclose(got.fun, ref.fun, rtol=1e-6) and np.allclose(got.x, ref.x, rtol=1e-5, atol=1e-6 * (hi - lo))


# ---- 3. sx_cmaes_eval_penalized on narrow rows ---------------------------------------------------------------------------
EVAL_NS = (1, 2, 15, 16, 17, 33, 64, 65, 128, 129, 255, 256, 257, 512, 513, 1024, "W-1", "W")  # W = sx_wide_from()
EVAL_PS = (1, 7, 33, 70)
KINDS = ("inside", "below", "above", "edges", "one@0", "one@lpr-1", "one@lpr", "one@last", "nan", "+inf", "-inf", "mixed")


def lanes_per_row(n):
    return 16 if n <= 64 else (32 if n <= 128 else 64)


def eval_inputs(n, P):
    """xm, xstd with no two elements equal, v with zeros, and P rows that walk through KINDS (starting at kind n, so that the
    short populations see every kind over the row lengths)."""
    rs = np.random.RandomState(1000 * P + n)
    xm, xstd = rs.permutation(np.linspace(-1.0, 1.0, n)), rs.permutation(np.linspace(0.5, 2.0, n))
    v = rs.uniform(0.1, 2.0, n)
    v[1::4] = 0.0
    zero, nonzero = np.flatnonzero(v == 0.0), np.flatnonzero(v != 0.0)
    X = rs.uniform(-0.95, 0.95, (P, n))
    lpr = lanes_per_row(n)
    for r in range(P):
        kind = KINDS[(r + n) % len(KINDS)]
        sign = 1.0 if r % 2 else -1.0
        if kind == "below":
            X[r] = rs.uniform(-3.0, -1.01, n)
        elif kind == "above":
            X[r] = rs.uniform(1.01, 3.0, n)
        elif kind == "edges":
            X[r, 0::3], X[r, 1::3], X[r, 2::3] = 1.0, -1.0, -0.0
        elif kind.startswith("one@"):
            at = {"0": 0, "lpr-1": lpr - 1, "lpr": lpr, "last": n - 1}[kind[4:]]
            X[r, min(at, n - 1)] = sign * 1.75
        elif kind == "nan":
            X[r, rs.randint(n)] = np.nan
        elif kind == "+inf":  # on a zero weight where there is one: inf * 0 = NaN
            X[r, zero[rs.randint(zero.size)] if zero.size else 0] = np.inf
        elif kind == "-inf":
            X[r, nonzero[rs.randint(nonzero.size)]] = -np.inf
        elif kind == "mixed":
            X[r] = rs.uniform(-1.6, 1.6, n)
    return X, xm, xstd, v


@pytest.mark.parametrize("n", EVAL_NS)
@pytest.mark.parametrize("name", ox.ALL)
def test_eval_penalized_narrow_rows(ctx, name, n):
    from stochopy_amd import _device, _lib

    t, p = _device.torch(), _device.ptr
    wide_from = _lib.wide_from()
    n = {"W-1": wide_from - 1, "W": wide_from}.get(n, n)
    fid = _lib.FUN_IDS[name]
    for P in EVAL_PS:
        X, xm, xstd, v = eval_inputs(n, P)
        dX, dxm, dxstd, dv = ctx.upload(X), ctx.upload(xm), ctx.upload(xstd), ctx.upload(v)
        f, pen, f0 = ctx.upload(np.full(P, -7.0)), ctx.upload(np.full(P, -7.0)), ctx.upload(np.full(P, -7.0))
        with t.cuda.stream(ctx.stream):
            _lib.check(ctx.L.sx_cmaes_eval_penalized(fid, p(dX), P, n, p(dxm), p(dxstd), p(dv), p(f), p(pen), ctx.stream_ptr))
            _lib.check(ctx.L.sx_cmaes_eval_penalized(fid, p(dX), P, n, p(dxm), p(dxstd), None, p(f0), None, ctx.stream_ptr))
        ctx.sync()
        f, pen, f0 = f.cpu().numpy(), pen.cpu().numpy(), f0.cpu().numpy()
        what = (name, n, P)
        pen_dev = check_penalty(pen, penalty_exact(X, v), n, what)
        inside = np.all(np.abs(X) <= 1.0, axis=1)
        assert np.array_equal(bits(pen[inside]), bits(np.zeros(int(inside.sum())))), what  # (exactly +0.0, -0.0 and +-1.0 included)
        ratio = check_objective(name, clip_keep_nan(X) * xstd + xm, f, what)
        assert np.array_equal(bits(f0), bits(f)), what
        print("penalize_eval %-16s n=%-4d P=%-2d pen=%.2e of %.2e  objective ratio=%.4f" % (name, n, P, pen_dev, (n + 4) * U, ratio))


# ---- 4. a NaN coordinate stays NaN through every clip of the resident loops ----------------------------------------------
@pytest.mark.parametrize("method,n", [("cmaes", 6), ("vdcma", 6), ("vdcma", "W+1"), ("vdcma", 4097)])
def test_nan_coordinate_survives_the_clips_of_the_resident_generation(sa, method, n):
    """One generation of the device-resident loop from a mean with a NaN coordinate, Penalize, return_all, maxiter = 1 (the
    stop step copies the best point): the reference's np.where(x < -1, -1, x) keeps the NaN, so every candidate's fitness,
    that coordinate of every recorded (clipped) candidate and of the best point are NaN -- not the lower bound.  The sites:
    the history kernel and the stop kernel's copy of CMA-ES and of VD-CMA (n = 6; n = sx_wide_from() + 1: the wide evaluation
    under the one-workgroup model update), and at n = 4097 -- VD-CMA's wide model, csrc/sx_vd_loop.hip -- the candidates' own
    clip in wide_vd_candidates_kernel and the copy in vw_h_phase."""
    from stochopy_amd import _lib
    from stochopy_amd.optimize._cmaes import _CmaDeviceRun
    from stochopy_amd.optimize._vdcma import _VdDeviceRun

    n = _lib.wide_from() + 1 if n == "W+1" else n
    P, bad = {6: 6, 4097: 56}.get(n, 32), 2  # (the spread history of 20 + 3 n / P entries must fit its 256 slots)
    lower, upper = np.full(n, 0.5), np.full(n, 3.0)
    x0 = np.linspace(1.0, 2.5, n)
    x0[bad] = np.nan
    Run = _CmaDeviceRun if method == "cmaes" else _VdDeviceRun
    run = Run(sa.factory.sphere.sx_id, lower, upper, x0, 1, P, 0.4, 0.5, 1e-12, 1e-30, 31, return_all=True, verbosity=1.0,
              penalize=True)
    run.step(1, *((0,) if method == "cmaes" else ()))  # (CMA-ES: no decomposition in this generation)
    run.ctx.sync()
    state = run.read_state()
    buf = {k: run.buffers[k].cpu().numpy() for k in ("fit", "hist_x", "hist_f", "xbest", "arx")}
    assert state.done == 1 and state.stop_it == 1
    assert np.isnan(buf["arx"][:, bad]).all() and np.isfinite(np.delete(buf["arx"], bad, axis=1)).all()
    assert np.isnan(buf["fit"]).all() and np.isnan(buf["hist_f"][0]).all()
    hx = buf["hist_x"][0]
    assert hx.shape == (P, n) and np.isnan(hx[:, bad]).all()
    rest = np.delete(hx, bad, axis=1)
    assert np.all(rest >= 0.5) and np.all(rest <= 3.0) and (np.abs(np.delete(buf["arx"], bad, axis=1)) > 1.0).any()
    assert np.isnan(buf["xbest"][bad]) and np.isfinite(np.delete(buf["xbest"], bad)).all()
