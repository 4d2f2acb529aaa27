"""GPU: the ensemble sampler's kernels (csrc/sx_sample_ensemble.hip, csrc/sx_sample_ensemble_moves.hip) on every objective, at
every row width, at the sizes where their passes and their LDS change, and on degenerate ensembles.  The tables, their x0
builders and the cached references live in tests/_ensemble_edges.py; tests/test_sample_ensemble_edges_host.py checks on the
restatement alone that the tables mean something and that the known answers asserted here are not taken from the device.

  A  all seven objectives x n = 1 ... 96 x both resident kernels (all 28 instantiations of ensemble_kernel<FUN, LPR> and
     ensemble_moves_kernel<FUN, LPR>), with idle row groups and ragged last passes, against the restatement at every sample
  B  W at the LDS limit (318 passes per half-sweep at n = 1) and either side of the 64 KiB dynamic-LDS attribute; a walker
     whose row group changes with the launch geometry is the same walker, bit for bit
  C  the propose / decide kernels around a caller's objective on 64-lane rows, both sides of the row-stride change
  D  walkers that coincide: the snooker guard and the DE move with equal donors, known answers bit for bit
  E  constraints="Reject" through ONE planted element, in every lane trip and at the row's end
  F  burn and thin where the passes and the 32-lane rows are

Tolerances: samples within 1e-9 of the range, values within 1e-6 relative, every count exact.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _ensemble_edges as edges  # noqa: E402
from test_gpu_sample_batched import device_objective  # noqa: E402

pytestmark = pytest.mark.gpu

SPAN = edges.SPAN
KEYS = ("x", "fun", "accept_ratio", "accept_ratios", "xall", "funall")


@pytest.fixture(scope="module")
def sa():
    import stochopy_amd

    return stochopy_amd


def run(sa, fun, n, x0=None, args=(), callback=None, **options):
    return sa.sample.sample(fun, edges.bounds(n), x0=x0, args=args, method="ensemble", callback=callback,
                            options=dict(options, rng="philox", backend="hip"))


def check(what, got, want):
    """The parities of the ensemble tests between a device run and the restated one; prints the case's figures first."""
    Cn, W = want.nacc.shape
    total = Cn * W * (want.nit - 1)
    with np.errstate(all="ignore"):
        dx = np.nanmax(np.abs(got.xall - want.xall)) / SPAN
        df = np.nanmax(np.abs(got.funall - want.funall) / np.abs(want.funall), initial=0.0)
    print(f"\n{what}: max |dx| / range {dx:.3g}, max rel df {df:.3g}, accepted {int(want.nacc.sum())} of {total}, "
          f"infeasible {total - int(want.nfeas.sum())}")
    assert got.nit == want.nit and got.walkers == W == want.walkers
    assert got.xall.shape == want.xall.shape and got.funall.shape == want.funall.shape
    assert np.array_equal(got.accept_ratios, want.accept_ratios)  # nacc / maxiter: the counts, exactly
    assert got.accept_ratio == want.accept_ratio
    if "nreject" in want:
        assert got.nreject == want.nreject
    else:
        assert "nreject" not in got
    if "moves" in want:
        assert got.moves == want.moves and (got.burn, got.thin) == (want.burn, want.thin)
    assert np.all(np.isfinite(got.funall))
    assert edges.agrees(got, want)


def same_bits(a, b, keys=KEYS):
    for key in keys:
        assert np.array_equal(a[key], b[key]), key


# ---- A ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", edges.A_CASES, ids=edges.case_id)
def test_every_objective_at_every_row_width(sa, case):
    """3 ensembles of W = 2 n + 4 walkers (192 at n = 96), 30 samples, compared at every sample: row_objective<FUN, LPR> under
    the divergence of `if (i < h)` -- idle row groups at h = 5 and 10, ragged last passes of 2 or 3 rows from h = 18 on."""
    name, n, kernel = case
    seed, want = edges.a_reference(case)
    got = run(sa, getattr(sa.factory, name), n, **dict(edges.a_options(case), seed=seed))
    check(f"A {edges.case_id(case)} W {want.walkers} seed {seed}", got, want)
    assert 0 < int(want.nacc.sum()) < want.nacc.size * (edges.A_MAXITER - 1)  # both outcomes of the decision
    if kernel == "moves":
        assert set(np.unique(want.kinds[:, 1:])) == {0, 1, 2, 3}  # every entry within the 30 samples
    if edges.flat(name, n):
        assert np.all(got.xall >= edges.LOWER) and np.all(got.xall <= edges.UPPER) and not got.funall.any()


# ---- B ------------------------------------------------------------------------------------------------------------------
def test_the_walkers_of_section_b_are_the_entry_points(sa):
    """The shapes of the table are computed from a restated byte count: it is sx_sample_ensemble_lds_bytes at every shape of
    the tables, the largest W are the largest that the entry point admits (W + 2 is refused), and the pair at n = 16 straddles
    the 64 KiB above which the launch sets the dynamic-LDS attribute."""
    from stochopy_amd import _lib
    from stochopy_amd.sample import _ensemble

    L = _lib.lib()
    for n, W in edges.B_SHAPES + tuple((n, edges.a_walkers(n)) for n in edges.A_NS) + tuple((n, 2 * n + 4) for n in edges.A_NS):
        assert L.sx_sample_ensemble_lds_bytes(W, n) == edges.lds_bytes(W, n), (n, W)
    assert edges.a_walkers(96) == 192 and all(edges.a_walkers(n) == 2 * n + 4 for n in edges.A_NS if n != 96)
    for n, W in edges.B_LARGEST.items():
        assert _ensemble.largest_walkers(n) == W
        assert 0 < L.sx_sample_ensemble_lds_bytes(W, n) <= edges.LDS_LIMIT < L.sx_sample_ensemble_lds_bytes(W + 2, n)
        for options in (edges.kernel_options(k) for k in edges.KERNELS):
            with pytest.raises(ValueError, match="walkers"):
                run(sa, sa.factory.rastrigin, n, maxiter=2, walkers=W + 2, chains=1, seed=1, **options)
    below, above = edges.B_LINE
    assert L.sx_sample_ensemble_lds_bytes(below, 16) <= 64 * 1024 < L.sx_sample_ensemble_lds_bytes(above, 16)
    assert above == below + 2


@pytest.mark.parametrize("case", edges.B_CASES, ids=edges.case_id)
def test_far_more_walkers_than_row_groups(sa, case):
    """2 ensembles, 12 samples: hundreds of passes per half-sweep over 16 row groups, and the two sides of 64 KiB."""
    name, n, W, kernel = case
    seed, want = edges.b_reference(case)
    got = run(sa, getattr(sa.factory, name), n, **dict(edges.b_options(case), seed=seed))
    check(f"B {edges.case_id(case)} passes {edges.passes(W, n)[0]} seed {seed}", got, want)


@pytest.mark.parametrize("kernel", edges.KERNELS)
@pytest.mark.parametrize("name", ["rastrigin", "ackley"])
def test_a_walker_at_the_lds_limit_does_not_depend_on_the_launch(sa, name, kernel):
    """(8, 2246): ensemble 1 of 2 is ensemble 1 of 9, and a run cut into one launch per sample by a callback (the state through
    sx_sample_args and back into LDS) is the run in one launch -- bit for bit."""
    n, W = edges.B_GEOMETRY
    case = (name, n, W, kernel)
    seed, want = edges.b_reference(case)
    o = dict(edges.b_options(case), seed=seed)
    fun = getattr(sa.factory, name)
    few = run(sa, fun, n, **o)
    many = run(sa, fun, n, **dict(o, chains=edges.B_MANY))
    for key in ("xall", "funall", "accept_ratios"):
        assert np.array_equal(few[key][1], many[key][1]), key
    seen = []
    cut = run(sa, fun, n, **o, callback=lambda xk, state: seen.append(np.array(xk, copy=True)))
    assert len(seen) == edges.B_MAXITER and np.array_equal(np.stack(seen, axis=1), few.xall)
    same_bits(cut, few)
    assert 0.0 < few.accept_ratios[1].mean() < (edges.B_MAXITER - 1) / edges.B_MAXITER  # (the state that round-trips moved)
    assert edges.agrees(few, want)


# ---- C ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", edges.C_CASES, ids=edges.case_id)
def test_whole_wave_rows_around_a_callers_objective(sa, case):
    """A torch objective through factory.batched on rows of 64 lanes, W = 2 n: the propose and decide kernels of both entry
    families, with the walkers in device memory."""
    import torch

    n, kernel = case
    seed, want = edges.c_reference(case)
    fun = sa.factory.batched(lambda X, c, s: (s * (X - c) ** 2).sum(dim=1))
    got = run(sa, fun, n, args=(torch.tensor(edges.c_centre(n), device="cuda"), edges.C_SCALE),
              **dict(edges.c_options(case), seed=seed))
    check(f"C {edges.case_id(case)} seed {seed}", got, want)
    with pytest.raises(ValueError, match="walkers"):  # (no resident form of such a row)
        run(sa, sa.factory.sphere, n, **dict(edges.c_options(case), seed=seed))


# ---- D ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", edges.D_CASES, ids=edges.case_id)
def test_a_whole_ensemble_on_one_point_stays_there(sa, case):
    """Every walker of ensemble g on p_g: the DE difference and the snooker move's dd are exactly 0 (the guard: c = 0, where
    0 / 0 would put NaN into every later sample), the stretch move proposes the partner.  Every sample is p_g bit for bit and
    the values are one constant per ensemble; "de" + "snooker" alone accept every proposal (d = 0), with FOUR the counts are the
    restatement's; resident and around a caller's objective."""
    n, W, name, moves = case
    seed, want = edges.d_whole_reference(case)
    x0, p = edges.d_x0_whole(n, W), edges.d_points(n)
    o = dict(edges.d_options(n, W, moves), seed=seed)
    m = edges.D_MAXITER
    resident = run(sa, getattr(sa.factory, name), n, x0=x0, **o)
    batched = run(sa, device_objective(sa, name), n, x0=x0, **o)
    for form, got in (("resident", resident), ("batched", batched)):
        assert np.array_equal(got.xall, np.broadcast_to(p[:, None, None, :], got.xall.shape)), form
        assert not np.isnan(got.funall).any() and np.all(got.funall == got.funall[:, :1, :1]), form
        if moves == "pair":
            assert np.all(got.accept_ratios == (m - 1) / m), form
        check(f"D whole {edges.case_id(case)} {form} seed {seed}", got, want)
    same_bits(batched, resident)


@pytest.mark.parametrize("shape", edges.D_SHAPES, ids=edges.case_id)
def test_one_half_on_one_point_leaves_the_first_sample_of_the_other_in_place(sa, shape):
    """Walkers [h, W) on p_g, "de" + "snooker": in the first half-sweep every donor difference and every snooker projection is
    exactly 0, so sample 1 of the walkers [0, h) is their sample 0 bit for bit and every one of those proposals is accepted;
    the run goes on from there against the restatement."""
    n, W, name = shape
    h = W // 2
    seed, want = edges.d_half_reference(shape)
    x0 = edges.d_x0_half(n, W)
    o = dict(edges.d_options(n, W, "pair"), seed=seed)
    resident = run(sa, getattr(sa.factory, name), n, x0=x0, **o)
    batched = run(sa, device_objective(sa, name), n, x0=x0, **o)
    for form, fun, got in (("resident", getattr(sa.factory, name), resident), ("batched", device_objective(sa, name), batched)):
        assert np.array_equal(got.xall[:, 0], x0), form
        assert np.array_equal(got.xall[:, 1, :h], got.xall[:, 0, :h]) and np.array_equal(got.funall[:, 1, :h], got.funall[:, 0, :h])
        first = run(sa, fun, n, x0=x0, **dict(o, maxiter=2))
        assert np.all(first.accept_ratios[:, :h] == 0.5), form  # one accepted proposal in two samples
        assert np.array_equal(first.accept_ratios, edges.d_half_first_sample(shape).accept_ratios), form
        check(f"D half {edges.case_id(shape)} {form} seed {seed}", got, want)
    same_bits(batched, resident)


# ---- E ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", edges.E_CASES, ids=edges.case_id)
def test_reject_through_one_planted_element(sa, case):
    """sphere with every walker zero but element e*: a proposal leaves the box through e* or not at all, so a row_in_box on
    the staged proposal that skips e* (a lane, a trip, the last element) counts other rejections than the restatement."""
    n, e, kernel = case
    seed, want, proposals = edges.e_reference(case)
    distance = np.minimum(np.abs(proposals[:, :, e] - edges.LOWER), np.abs(proposals[:, :, e] - edges.UPPER))
    assert distance.min() > edges.E_MARGIN * SPAN  # (no decision hangs on the last bits of a product)
    assert 0 < want.nreject < edges.e_total(n)
    got = run(sa, sa.factory.sphere, n, x0=edges.e_x0(n, e), **dict(edges.e_options(case), seed=seed))
    check(f"E {edges.case_id(case)} seed {seed}", got, want)
    assert np.all(got.xall >= edges.LOWER) and np.all(got.xall <= edges.UPPER)
    assert not np.delete(got.xall, e, axis=-1).any()


# ---- F ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("external", [False, True], ids=["resident", "batched"])
@pytest.mark.parametrize("shape", edges.F_SHAPES, ids=edges.case_id)
def test_burn_and_thin_record_rows_of_the_same_run(sa, shape, external):
    """(17, 38): two passes, the second of 3 rows; (65, 134): 32-lane rows, five passes.  The recorded rows are rows of the run
    that records everything, bit for bit; the counts and the best values run over all samples."""
    n, W, name = shape
    seed, want = edges.f_reference(shape)
    o = dict(edges.f_options(shape), seed=seed)
    fun = device_objective(sa, name) if external else getattr(sa.factory, name)
    form = "batched" if external else "resident"
    full = run(sa, fun, n, **o)
    check(f"F {edges.case_id(shape)} {form} seed {seed}", full, want)
    for burn, thin in edges.F_CUTS:
        recorded = np.arange(burn, edges.F_MAXITER, thin)
        cut = run(sa, fun, n, burn=burn, thin=thin, **o)
        assert cut.xall.shape == (edges.F_ENSEMBLES, len(recorded), W, n) and (cut.burn, cut.thin) == (burn, thin)
        assert np.array_equal(cut.xall, full.xall[:, recorded]) and np.array_equal(cut.funall, full.funall[:, recorded])
        same_bits(cut, full, ("x", "fun", "accept_ratio", "accept_ratios"))  # over all samples
        check(f"F {edges.case_id(shape)} {form} burn {burn} thin {thin}", cut, edges.restate(name, n, None, dict(o, burn=burn, thin=thin)))
