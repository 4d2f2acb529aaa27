"""The planted states of tests/test_gpu_penalize.py on the CPU (tests/_penalize_abi.py): the long-double restatement and
oracle.engine.PenalizeState agree on every case's flags, history and grown coordinates; the growth comparisons keep their
distance from the threshold, so that double and long double decide alike; the kernel's quartile rule stated in numpy is
np.percentile bit for bit on the planted fitness vectors; and the table visits the branches it is there for."""
import numpy as np
import pytest

import _penalize_abi as pa

LD = np.longdouble
needs_longdouble = pytest.mark.skipif(np.finfo(LD).nmant < 63, reason="np.longdouble has fewer than 63 mantissa bits here")
MARGIN = 1e-9


def bits(a):
    return np.asarray(a, dtype=np.float64).view(np.int64)


def test_constants_read_from_the_source():
    assert pa.PATH_THREADS == 1024 and pa.HIST == 256
    assert pa.admitted(470, 6) and pa.cap(470, 6) == 255.0 and not pa.admitted(472, 6)
    assert pa.cap(4, 6) == 22.0 and pa.cap(6, 12) == 21.5
    ns = {c.n for c in pa.cases().values()}
    assert {pa.PATH_THREADS - 1, pa.PATH_THREADS, pa.PATH_THREADS + 1, 1, 2, 63, 64, 65} <= ns


@pytest.mark.parametrize("tag", pa.tags())
def test_double_restatement_is_the_oracle(tag):
    """In float64 the restatement IS oracle.engine.PenalizeState.apply: flags, history, weights and grown set."""
    case = pa.cases()[tag]
    st, fit, clipped = pa.oracle_apply(case)
    r = pa.restate(case, np.float64)
    assert (st.dfithist.size, int(st.validfitval), int(st.iniphase)) == (r.count, r.valid, r.ini)
    assert np.array_equal(bits(st.dfithist[:-1]), bits(r.hist[:-1]))
    assert np.isclose(st.dfithist[-1], float(r.hist[-1]), rtol=8 * pa.U * case.n, atol=0.0) or not r.fresh
    if not r.fresh:
        assert bits(st.dfithist[-1]) == bits(r.hist[-1])
    assert np.allclose(st.weights, r.w.astype(np.float64), rtol=8 * pa.U * case.n, atol=0.0)
    base = np.full(case.n, float(r.fill)) if r.filled else case.w
    assert np.array_equal(st.weights > base * (1.0 + 1e-6), r.grown)  # (the growth factor is at least 1.2^(1/20 n) ... > 1 + 1e-6 here)
    assert np.array_equal(clipped, np.clip(case.arx, -1.0, 1.0))


@needs_longdouble
@pytest.mark.parametrize("tag", pa.tags())
def test_long_double_and_double_decide_alike(tag):
    case = pa.cases()[tag]
    a, b = pa.restate(case, np.float64), pa.restate(case, LD)
    assert (a.count, a.valid, a.ini, a.filled, a.fresh) == (b.count, b.valid, b.ini, b.filled, b.fresh)
    assert np.array_equal(a.grown, b.grown) and np.array_equal(a.outside, b.outside)
    assert a.margin >= MARGIN and b.margin >= MARGIN, (a.margin, b.margin)
    if a.grown.any():
        assert float(b.fac) > 1.0 + 1e-5  # a grown weight cannot be mistaken for an untouched one


@pytest.mark.parametrize("tag", pa.tags())
def test_kernel_quartile_rule_is_numpys(tag):
    fit = pa.cases()[tag].fit
    assert np.array_equal(bits(pa.kernel_quartiles(fit)), bits(np.percentile(fit, [25.0, 75.0])))


def test_quartile_rule_on_every_popsize_and_on_ties():
    rs = np.random.RandomState(5)
    for P in list(range(2, 40)) + [70, 257]:
        for fit in (rs.uniform(-1e3, 1e3, P), rs.randint(0, 3, P).astype(np.float64), np.exp(rs.uniform(-40, 40, P))):
            assert np.array_equal(bits(pa.kernel_quartiles(fit)), bits(np.percentile(fit, [25.0, 75.0]))), (P, fit)


def test_the_table_visits_its_branches():
    cs = pa.cases()
    out = {t: pa.restate(c, np.float64) for t, c in cs.items()}
    for form in pa.FORMS:
        r = out["first-inside-" + form]
        assert (r.count, r.valid, r.ini, r.fresh, r.filled) == (1, 1, 1, True, False)
        r = out["first-outside-" + form]
        assert (r.count, r.valid, r.ini, r.filled) == (1, 1, 1, True) and r.fill == 2.0002 * r.delta
        for t in ("flat-all-", "flat-middle-"):
            r = out[t + form]
            assert (r.count, r.valid, r.fresh, float(r.delta)) == (2, 0, False, 1.0)
        r = out["flat-mixed-" + form]
        assert (r.count, r.fresh, float(r.delta)) == (8, False, 0.5)
        for n, P in ((4, 6), (6, 12)):  # count after the call: pushed below the cap, shifted from it on
            got = [out["window-%s-n%d-c%d" % (form, n, c)].count for c in (20, 21, 22, 23)]
            assert got == [21, 22, 22, 23]
            r, c = out["window-%s-n%d-c22" % (form, n)], cs["window-%s-n%d-c22" % (form, n)]
            assert np.array_equal(bits(r.hist[:-1]), bits(c.hist[1:]))  # shifted, in order
        assert [out["largest-%s-c%d" % (form, c)].count for c in (253, 254, 255)] == [254, 255, 255]
        g = out["growth-" + form]
        assert g.grown.tolist() == [False, True, False, False, False, False, True, False]
        assert g.outside.tolist() == [False, True, True, True, True, True, True, True] and not g.filled
        # ini falls only with valid set (before or in this call), gen > 2 and a coordinate outside
        for t, r in out.items():
            if t.startswith("phase-" + form):
                c = cs[t]
                fell = c.ini == 1 and r.ini == 0
                assert fell == (c.ini == 1 and r.valid == 1 and c.gen > 2 and bool(r.outside.any())), t
                assert r.filled == (c.ini == 1 and bool(r.outside.any())), t
        assert any(t.startswith("phase-" + form) and c.valid == 0 and out[t].valid == 0 for t, c in cs.items())
        assert any(t.startswith("phase-" + form) and c.valid == 0 and out[t].valid == 1 and out[t].count == 1 for t, c in cs.items())
        # the fill and the growth in one call, growing and not growing coordinates side by side, on each side of the stride
        for n in (65, pa.PATH_THREADS + 1):
            r = out["shape-%s-n%d-P70" % (form, n)]
            assert r.filled and r.grown.any() and (r.outside & ~r.grown).any()
            assert r.grown[:pa.PATH_THREADS].any() and (n <= pa.PATH_THREADS or r.outside[pa.PATH_THREADS:].any())
        d = pa.diagonal(cs["span-" + form])
        assert d.min() < 1.1e-8 and d.max() > 0.9


def test_quartile_index_kinds():
    """(P - 1) q: integral at P = 5, fractions on both sides of 1/2 among the others; at P = 2 the upper neighbour is the last
    entry (the clamp `hi = P - 1` itself can act only on an integral index P - 1, which q < 1 never gives)."""
    frac = {P: ((P - 1) * 0.25) % 1.0 for P in pa.PS}
    assert frac[5] == 0.0 and any(0.0 < f < 0.5 for f in frac.values()) and any(f >= 0.5 for f in frac.values())
    assert int(np.floor(1 * 0.75)) + 1 == 2 - 1
    assert all(int(np.floor((P - 1) * 0.75)) + 1 <= P - 1 for P in range(2, 300))
