"""The conditions the tables of tests/_ensemble_edges.py rest on, checked on the numpy restatements alone (no GPU): every entry
is admitted, both outcomes of the decision and every move occur where a section says so, the known answers that
tests/test_gpu_sample_ensemble_edges.py asserts on the device hold in the restatement (they are not taken from the device), no
feasibility test hangs on the last bits of a proposal, and section A would notice an objective that lost an element."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _ensemble_edges as edges  # noqa: E402


def proposals_of(want):
    Cn, W = want.nacc.shape
    return Cn * W * (want.nit - 1)


def test_the_shapes_are_the_ones_the_tables_are_chosen_for():
    """The byte counts by the formula: the largest W at n = 1, 8, 33, the pair either side of 64 KiB, and section A's W with the
    divergence it is there for."""
    assert edges.B_LARGEST == {1: 10168, 8: 2246, 33: 582} and edges.B_LINE == (458, 460)
    for n, W in edges.B_LARGEST.items():
        assert edges.lds_bytes(W, n) <= edges.LDS_LIMIT < edges.lds_bytes(W + 2, n)
    assert edges.lds_bytes(458, 16) <= 64 * 1024 < edges.lds_bytes(460, 16)
    assert edges.passes(10168, 1) == (318, 12)
    assert [edges.a_walkers(n) for n in edges.A_NS] == [6, 10, 20, 36, 38, 68, 70, 132, 134, 192]
    assert edges.lds_bytes(196, 96) > edges.LDS_LIMIT >= edges.lds_bytes(192, 96)
    # h = 3, 5, 10: one pass with idle row groups in the last wave (4 row groups to a wave); then ragged last passes of 2 or 3 rows
    assert [edges.passes(edges.a_walkers(n), n) for n in edges.A_NS] == [(1, 3), (1, 5), (1, 10), (2, 2), (2, 3), (3, 2), (3, 3), (5, 2),
                                                                         (5, 3), (6, 16)]
    assert len(edges.A_CASES) == 7 * 10 * 2 and {c[0] for c in edges.A_CASES} == set(edges.ALL)
    assert {edges.lanes_per_row(c[1]) for c in edges.A_CASES} == {16, 32}  # 7 objectives x 2 lane layouts x 2 kernels = 28
    # section E's planted elements by (lane, trip): the last lane, the first element of a later trip, the row's end
    assert [lanes_e(n, e) for n, e in edges.E_PAIRS] == [(15, 0), (0, 1), (0, 2), (15, 3), (31, 0), (0, 1), (0, 2), (31, 2)]


@pytest.mark.parametrize("kernel", edges.KERNELS)
@pytest.mark.parametrize("name", edges.ALL)
def test_section_a_is_admitted_decides_both_ways_and_discriminates(name, kernel):
    for n in edges.A_NS:
        case = (name, n, kernel)
        seed, want = edges.a_reference(case)
        assert 700 + n <= seed < 700 + n + 8 and want.xall.shape == (edges.A_ENSEMBLES, edges.A_MAXITER, edges.a_walkers(n), n)
        assert np.all(np.isfinite(want.funall))
        assert 0 < int(want.nacc.sum()) < proposals_of(want), case  # both outcomes of the decision
        if kernel == "moves":
            assert set(np.unique(want.kinds[:, 1:])) == {0, 1, 2, 3}, case  # every entry within the 30 samples
        if edges.flat(name, n):
            # nothing but the box rejects: every feasible proposal is accepted (d = 0.0 exactly)
            assert want.nreject > 0 and np.array_equal(want.nacc, want.nfeas) and not want.funall.any()
        else:
            assert "nreject" not in want
        if n >= 3:
            for e in edges.blind_elements(n):
                assert edges.a_discriminates(case, e), (case, e)
    assert edges.blind_elements(96) == (16, 32, 95) and edges.blind_elements(17) == (16,) and edges.blind_elements(3) == (2,)


def test_section_b_is_admitted_and_decides_both_ways():
    for case in edges.B_CASES:
        seed, want = edges.b_reference(case)
        assert edges.B_SEED <= seed < edges.B_SEED + 8 and np.all(np.isfinite(want.funall))
        assert 0 < int(want.nacc.sum()) < proposals_of(want), case
        each = want.nacc.sum(axis=1)
        assert np.all((0 < each) & (each < proposals_of(want) // edges.B_ENSEMBLES)), case  # in each ensemble
        if case[3] == "moves":
            assert len(set(np.unique(want.kinds[:, 1:]))) == 4, case


def test_section_c_is_admitted_and_decides_both_ways():
    for case in edges.C_CASES:
        n, kernel = case
        seed, want = edges.c_reference(case)
        assert edges.C_SEED <= seed < edges.C_SEED + 8 and want.xall.shape[1:] == (4 if n == 1030 else 8, 2 * n, n)
        assert 0 < int(want.nacc.sum()) < proposals_of(want), case
        if kernel == "moves":
            kinds = {edges.FOUR[k][0] for k in np.unique(want.kinds[:, 1:])}
            assert kinds >= {"de", "snooker"}, case
    # (600 and 1030 draw no stretch entry in their 14 and 6 draws; 129, 256 and 257 draw all four)
    assert all(len(set(np.unique(edges.c_reference((n, "moves"))[1].kinds[:, 1:]))) == 4 for n in (129, 256, 257))


@pytest.mark.parametrize("case", edges.D_CASES, ids=edges.case_id)
def test_a_whole_ensemble_on_one_point_stays_there(case):
    n, W, name, moves = case
    p = edges.d_points(n)
    assert np.all(p != 0.0) and all(len(set(row)) == n for row in p) and len({tuple(row) for row in p}) == edges.D_ENSEMBLES
    assert np.all(np.abs(p) < edges.UPPER)
    x0 = edges.d_x0_whole(n, W)
    assert x0.shape == (edges.D_ENSEMBLES, W, n) and np.array_equal(x0, np.broadcast_to(p[:, None, :], x0.shape))
    seed, want = edges.d_whole_reference(case)
    m = edges.D_MAXITER
    assert np.array_equal(want.xall, np.broadcast_to(p[:, None, None, :], want.xall.shape))  # bit for bit
    assert not np.isnan(want.funall).any() and np.all(want.funall == want.funall[:, :1, :1])
    if moves == "pair":
        assert np.all(want.accept_ratios == (m - 1) / m)  # d = 0 accepts
        assert set(np.unique(want.kinds[:, 1:])) == {0, 1}
    else:
        assert set(np.unique(want.kinds[:, 1:])) == {0, 1, 2, 3}
        # the stretch entry proposes the partner, which is p too, and decides on z^(n - 1) alone: it rejects
        assert np.all(want.nacc <= m - 1) and 0 < int(want.nacc.sum()) < proposals_of(want)


@pytest.mark.parametrize("shape", edges.D_SHAPES, ids=edges.case_id)
def test_one_half_on_one_point_leaves_the_first_sample_of_the_other_in_place(shape):
    n, W, name = shape
    h = W // 2
    x0, p = edges.d_x0_half(n, W), edges.d_points(n)
    assert np.array_equal(x0[:, h:], np.broadcast_to(p[:, None, :], (edges.D_ENSEMBLES, h, n)))
    assert len(np.unique(x0[:, :h])) == edges.D_ENSEMBLES * h * n and np.all(np.abs(x0) <= edges.UPPER)
    seed, want = edges.d_half_reference(shape)
    assert np.array_equal(want.xall[:, 0], x0)
    assert np.array_equal(want.xall[:, 1, :h], want.xall[:, 0, :h]) and np.array_equal(want.funall[:, 1, :h], want.funall[:, 0, :h])
    first = edges.d_half_first_sample(shape)
    assert np.array_equal(first.xall, want.xall[:, :2]) and np.all(first.nacc[:, :h] == 1)  # every one of them accepted
    assert set(np.unique(want.kinds[:, 1:])) == {0, 1}
    assert not np.array_equal(want.xall[:, 1, h:], want.xall[:, 0, h:])  # the half on p moves against the other
    assert 0 < int(want.nacc.sum()) < proposals_of(want) and np.all(np.isfinite(want.funall))


@pytest.mark.parametrize("case", edges.E_CASES, ids=edges.case_id)
def test_reject_cases_reject_through_the_planted_element(case):
    n, e, kernel = case
    x0 = edges.e_x0(n, e)
    assert not np.delete(x0, e, axis=1).any()
    planted = np.abs(x0[:, e])
    assert planted.min() == 0.5 * edges.UPPER and planted.max() == edges.UPPER * (1.0 - 1.0e-9) < edges.UPPER
    for half in (x0[:n, e], x0[n:, e]):
        assert (half > 0).any() and (half < 0).any()
    seed, want, proposals = edges.e_reference(case)
    total = edges.e_total(n)
    print(case, "seed", seed, "rejected", want.nreject, "of", total)
    assert 41 + n + e <= seed < 41 + n + e + 8
    assert 0 < want.nreject < total and proposals.shape == (2 * (edges.E_MAXITER - 1), edges.E_ENSEMBLES * n, n)
    assert not np.delete(proposals, e, axis=2).any()  # every move stays on the line
    outside = (proposals[:, :, e] < edges.LOWER) | (proposals[:, :, e] > edges.UPPER)
    assert int(outside.sum()) == want.nreject
    distance = np.minimum(np.abs(proposals[:, :, e] - edges.LOWER), np.abs(proposals[:, :, e] - edges.UPPER))
    assert distance.min() > edges.E_MARGIN * edges.SPAN
    assert np.all(want.xall >= edges.LOWER) and np.all(want.xall <= edges.UPPER)
    assert 0 < int(want.nacc.sum()) < int(want.nfeas.sum())  # feasible proposals are accepted and rejected
    if kernel == "moves":
        assert set(np.unique(want.kinds[:, 1:])) == {0, 1, 2, 3}


def lanes_e(n, e):
    """(lane, trip) of element e in its row."""
    lpr = edges.lanes_per_row(n)
    return e % lpr, e // lpr


def test_section_f_is_admitted_and_uses_every_move():
    for shape in edges.F_SHAPES:
        n, W, name = shape
        seed, want = edges.f_reference(shape)
        assert 31 + n <= seed < 31 + n + 8
        assert set(np.unique(want.kinds[:, 1:])) == {0, 1, 2, 3} and 0 < int(want.nacc.sum()) < proposals_of(want)
        for burn, thin in edges.F_CUTS:
            cut = edges.restate(name, n, None, dict(edges.f_options(shape), seed=seed, burn=burn, thin=thin))
            recorded = np.arange(burn, edges.F_MAXITER, thin)
            assert np.array_equal(cut.xall, want.xall[:, recorded]) and np.array_equal(cut.nacc, want.nacc) and cut.fun == want.fun
    assert [len(np.arange(b, edges.F_MAXITER, t)) for b, t in edges.F_CUTS] == [8, 1, 15]
