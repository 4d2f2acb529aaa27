"""GPU: the sampler kernels (csrc/sx_sample.hip, sx_sample_unfused.hip, the gradient and Box-Muller helpers of sx_sample.hpp
and sx_device.hpp) at every row width and on every objective.  The tables, their x0 builders and the cached references live
in tests/_sample_edges.py; tests/test_sample_edges_host.py checks on the restatement alone that the tables mean something.

  A  sx_sample_gradient per element against the closed forms, all seven objectives, n = 1 ... 2048, planted rows
  B  short hmc chains (4 samples, 2 leaps) against the restatement: analytic and finite-difference gradients, all seven
     objectives, all three lane layouts, both row strides, per-chain x0; x within 1000 times the restatement's own one-ulp
     deviation (profiles/sample_edges_sensitivity.txt), never more than the project's 1e-6 of the range
  C  finite differences around a caller's objective beyond one trip of the lanes: the fused run, bit for bit
  D  constraints="Reject" through ONE planted element, in every lane trip and at the row's end
  E  mcmc against the restatement where the Box-Muller pairing, the lane count and the block start change
  F  a run cut into one launch per sample is the whole run, on wide rows
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _sample_edges as edges  # noqa: E402
from test_gpu_sample_batched import assert_same_run, both  # noqa: E402

pytestmark = pytest.mark.gpu

SPAN = edges.SPAN


@pytest.fixture(scope="module")
def sa():
    import stochopy_amd

    return stochopy_amd


def close_samples(got, want, xtol=edges.PROJECT_XTOL):
    return np.allclose(got, want, rtol=0, atol=xtol * SPAN)


def close_values(got, want):
    return np.allclose(got, want, rtol=1e-6, atol=0)


# ---- A ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", edges.GRAD_NS)
@pytest.mark.parametrize("objective", edges.ALL)
def test_gradient_per_element(sa, objective, n):
    """Grad<FUN> through sx_sample_gradient (the hmc kernel's grad_apply) on 33 rows: every row within 1e-12 of the closed
    form's norm; a row whose gradient is identically zero (ackley's origin branch, rosenbrock at its minimum and at n = 1,
    the even objectives at 0) exactly 0.0 in every element."""
    import torch

    from stochopy_amd import _device, _lib

    X, want = edges.gradient_rows(objective, n), edges.gradient_reference(objective, n)
    ctx = _device.Context()
    with torch.cuda.stream(ctx.stream):
        dX = ctx.upload(np.ascontiguousarray(X))
        dG = ctx.empty((edges.GRAD_ROWS, n))
        dG.fill_(float("nan"))  # (an element the kernel skipped cannot pass)
        _lib.check(ctx.L.sx_sample_gradient(_lib.FUN_IDS[objective], _device.ptr(dX), edges.GRAD_ROWS, n, _device.ptr(dG),
                                            ctx.stream_ptr), "sx_sample_gradient")
        G = dG.cpu().numpy()
    norm = np.linalg.norm(want, axis=1)
    zero = norm == 0.0
    err = np.linalg.norm(G - want, axis=1)
    with np.errstate(all="ignore"):
        print(f"\ngradient {objective} n = {n}: max relative error {np.max(err[~zero] / norm[~zero], initial=0.0):.3g}, "
              f"{int(zero.sum())} rows exactly zero")
    assert np.all(np.isfinite(G))
    assert not G[zero].any()
    assert np.all(err[~zero] <= edges.GRAD_RTOL * norm[~zero])
    if objective in ("ackley", "griewank", "quartic", "rastrigin", "sphere"):
        assert zero[0]
    if objective == "rosenbrock":
        assert zero[1] and (n > 1 or zero.all())


# ---- B ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", edges.HMC_CASES, ids=edges.hmc_id)
def test_short_hmc_chains_vs_restatement(sa, case):
    """24 chains, 4 samples, 2 leaps: counts exact, values within 1e-6 relative, samples within the case's own share of the
    range.  rosenbrock and quartic start from a per-chain x0 (x0_stride = n)."""
    name, n, jac = case
    want = edges.hmc_reference(case)
    xtol = edges.hmc_xtol(case)
    got = sa.sample.sample(getattr(sa.factory, name), edges.bounds(n), x0=edges.hmc_x0(name, n), method="hmc",
                           options=dict(edges.hmc_options(case), backend="hip"))
    assert got.xall.shape == want.xall.shape == (edges.HMC_CHAINS, edges.HMC_MAXITER, n)
    with np.errstate(all="ignore"):
        df = np.abs(got.funall - want.funall) / np.abs(want.funall)
        print(f"\nhmc {edges.hmc_id(case)}: max |dx| / range {np.abs(got.xall - want.xall).max() / SPAN:.3g} (bar {xtol:.3g}), "
              f"max rel df {np.nanmax(df, initial=0.0):.3g}, accepted {int(want.nacc.sum())} of 72")
    assert got.nit == want.nit == edges.HMC_MAXITER
    assert got.nfev == want.nfev
    assert np.array_equal(got.accept_ratios, want.accept_ratios) and got.accept_ratio == want.accept_ratio
    assert close_samples(got.xall, want.xall, xtol) and close_samples(got.x, want.x, xtol)
    assert close_values(got.funall, want.funall) and close_values(got.fun, want.fun)
    if name in edges.HMC_NARROW:
        assert np.array_equal(got.xall[:, 0], edges.hmc_x0(name, n))  # each chain starts at ITS row of x0


def test_short_hmc_chains_reject_too():
    """On the restatement: the full-box cases reject as well as accept (rastrigin at n <= 33 accepts 66 to 69 of 72), so both
    outcomes of the decision are compared above."""
    rejected = [72 - int(edges.hmc_reference(c).nacc.sum()) for c in edges.HMC_CASES if c[0] not in edges.HMC_NARROW]
    assert sum(rejected) > 0


# ---- C ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("objective,ndim,chains,axes", edges.FD_UNFUSED)
def test_finite_differences_beyond_one_lane_trip_are_the_fused_ones(sa, monkeypatch, objective, ndim, chains, axes):
    from stochopy_amd.sample import _chains

    if axes is not None:
        monkeypatch.setattr(_chains, "FD_STACK_BYTES", 2 * chains * ndim * 8 * axes)
        assert _chains.fd_axes_per_chunk(chains, ndim) == axes
    else:
        assert _chains.fd_axes_per_chunk(chains, ndim) == ndim
    opts = {"maxiter": 4, "nleap": 2, "stepsize": 0.01, "jac": None, "seed": 300 + ndim + chains, "chains": chains,
            "return_all": True}
    ext, fused = both(sa, "hmc", objective, ndim, opts)
    assert_same_run(ext, fused, chains, True)
    assert ext.nfev == chains * (1 + 3 * 2 * ndim * 4) + 2 * chains * 3


@pytest.mark.parametrize("objective,ndim,chains", edges.ANALYTIC_UNFUSED)
def test_a_batched_gradient_on_wide_rows_is_the_fused_analytic_run(sa, objective, ndim, chains):
    opts = {"maxiter": 4, "nleap": 2, "stepsize": 0.01, "jac": "analytic", "seed": 200 + ndim + chains, "chains": chains,
            "return_all": True}
    ext, fused = both(sa, "hmc", objective, ndim, opts)
    assert_same_run(ext, fused, chains, True)
    assert ext.nfev == chains + 2 * chains * 3


# ---- D ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", edges.REJECT_CASES, ids=lambda c: "-".join(map(str, c)))
def test_reject_through_one_planted_element(sa, case):
    """sphere from zeros with element e* a billionth inside its bound: a proposal leaves the box through e* or not at all, so
    a row_in_box that skips e* (a lane, a trip, the last element) counts other rejections than the restatement."""
    method, n, e = case
    want, proposals = edges.reject_reference(case)
    distance = np.minimum(np.abs(proposals[:, :, e] - edges.LOWER), np.abs(proposals[:, :, e] - edges.UPPER))
    assert distance.min() > edges.REJECT_MARGIN * SPAN  # (no decision hangs on the last bits of a normal)
    got = sa.sample.sample(sa.factory.sphere, edges.bounds(n), x0=edges.reject_x0(n, e), method=method,
                           options=dict(edges.reject_options(method), backend="hip"))
    want_rejected = edges.REJECT_TOTAL - int(want.nfeas.sum())
    print(f"\nreject {method} n = {n} e* = {e}: rejected as infeasible {got.nreject} (restatement {want_rejected}) of "
          f"{edges.REJECT_TOTAL}, max |dx| / range {np.abs(got.xall - want.xall).max() / SPAN:.3g}")
    assert 0 < want_rejected < edges.REJECT_TOTAL
    assert got.nreject == want_rejected
    assert np.array_equal(got.accept_ratios, want.accept_ratios)
    assert np.all(got.xall >= edges.LOWER) and np.all(got.xall <= edges.UPPER)
    assert close_samples(got.xall, want.xall) and close_values(got.funall, want.funall)


# ---- E ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", edges.MCMC_CASES, ids=edges.mcmc_id)
def test_mcmc_at_the_layout_edges_vs_restatement(sa, case):
    """The bars of test_gpu_sample.py test_parity_with_the_restatement_philox: 1e-6 of the range, 1e-6 relative, counts exact."""
    name, n, perc, chains = case
    want = edges.mcmc_reference(case)
    got = sa.sample.sample(getattr(sa.factory, name), edges.bounds(n), method="mcmc",
                           options=dict(edges.mcmc_options(case), backend="hip"))
    assert got.xall.shape == want.xall.shape == ((chains, edges.MCMC_MAXITER, n) if chains > 1 else (edges.MCMC_MAXITER, n))
    with np.errstate(all="ignore"):
        print(f"\nmcmc {edges.mcmc_id(case)}: max |dx| / range {np.abs(got.xall - want.xall).max() / SPAN:.3g}, max rel df "
              f"{np.nanmax(np.abs(got.funall - want.funall) / np.abs(want.funall), initial=0.0):.3g}, accept_ratio "
              f"{want.accept_ratio:.3g}")
    assert got.nit == want.nit
    if chains > 1:
        assert np.array_equal(got.accept_ratios, want.accept_ratios)
    assert got.accept_ratio == want.accept_ratio
    assert close_samples(got.xall, want.xall) and close_values(got.funall, want.funall)
    assert close_samples(got.x, want.x) and close_values(got.fun, want.fun)


# ---- F ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", edges.CUT_NS)
@pytest.mark.parametrize("method", ["mcmc", "hmc"])
def test_a_cut_run_is_the_whole_run_on_wide_rows(sa, method, n):
    """test_gpu_sample.py test_a_chain_does_not_depend_on_the_launch on rows of 130 and 300 elements: chain 5 of 7 is chain 5
    of 40, and one launch per sample (the state through sx_sample_args) is the run in one launch -- bit for bit."""
    m = edges.CUT_MAXITER
    opts = {"maxiter": m, "seed": 5, "rng": "philox", "backend": "hip"}
    # mcmc: blocks of int(0.3 n) variables, so an accepted sample copies a part of the row that starts inside a lane trip; with
    # these steps chain 5 accepts 4 to 9 of its 11 proposals in the restatement (the default step accepts next to none here)
    opts.update({"jac": "analytic"} if method == "hmc" else {"perc": 0.3, "stepsize": 0.02})
    fun = sa.factory.rastrigin
    few = sa.sample.sample(fun, edges.bounds(n), method=method, options=dict(opts, chains=edges.CUT_FEW))
    many = sa.sample.sample(fun, edges.bounds(n), method=method, options=dict(opts, chains=edges.CUT_MANY))
    assert np.all(np.isfinite(few.funall))
    assert np.array_equal(few.xall[5], many.xall[5]) and np.array_equal(few.funall[5], many.funall[5])
    assert few.accept_ratios[5] == many.accept_ratios[5]
    seen = []
    cut = sa.sample.sample(fun, edges.bounds(n), method=method, options=dict(opts, chains=edges.CUT_FEW),
                           callback=lambda xk, state: seen.append(np.array(xk, copy=True)))
    assert len(seen) == m and np.array_equal(np.stack(seen, axis=1), few.xall)
    assert np.array_equal(cut.xall, few.xall) and np.array_equal(cut.funall, few.funall)
    assert np.array_equal(cut.x, few.x) and cut.fun == few.fun and cut.accept_ratio == few.accept_ratio
    assert np.array_equal(cut.accept_ratios, few.accept_ratios)
    if method == "hmc":
        assert cut.nfev == few.nfev
    assert 0.0 < few.accept_ratios[5] < 1.0  # (the state that round-trips moved)
