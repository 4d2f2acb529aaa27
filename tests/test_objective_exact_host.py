"""tests/_objective_exact.py on the CPU: the long-double restatement of the seven objectives against mpmath at 40 digits,
numpy's own distance from it on every input of tests/test_gpu_objective_domains.py, and the inputs themselves."""
import numpy as np
import pytest

import _objective_exact as ox
from oracle.objectives import OBJECTIVES

pytestmark = pytest.mark.skipif(not ox.have_longdouble(),
                                reason="np.longdouble has fewer than 63 mantissa bits here: no reference finer than double")

CASES = [(name, n, kind) for name in ox.ALL for n in ox.NS for kind in ox.kinds(name)]


def test_planted_values_are_the_ones_a_hand_written_cosine_must_get_right():
    v = ox.planted_values()
    have = set(v.tolist())
    assert {0.0, 1.0e-300, 5.0e-324, 2.0 ** 52, 2.0 ** 53 + 2.0} <= have
    assert np.signbit(v[v == 0.0]).any() and not np.signbit(v[v == 0.0]).all()
    for k in (0, 1, 2, 255, 256, 599, 600):
        for x in (float(k), k + 0.5, k - 0.5, k + 0.25, k - 0.25):
            for s in (x, -x):
                assert {s, float(np.nextafter(s, np.inf)), float(np.nextafter(s, -np.inf))} <= have, s
    assert np.abs(v[np.abs(v) < ox.HUGE]).max() == np.nextafter(600.5, np.inf)


@pytest.mark.parametrize("name,n,kind", CASES)
def test_rows(name, n, kind):
    X = ox.rows(name, n, kind)
    assert X.shape[1] == n and X.shape[0] >= ox.ROWS and np.all(np.isfinite(X))
    big = ox.huge_rows(X)
    if kind == "own":
        assert np.abs(X).max() <= ox.DOMAIN[name] and np.abs(X).max() > 0.9 * ox.DOMAIN[name] * (n > 1)
    elif kind == "wide":
        assert np.abs(X).max() <= ox.WIDE and (n == 1 or np.abs(X).max() > 500.0)
    else:
        v = ox.planted_values()
        assert np.isin(v, X).all(), "every planted value sits in some row"
        assert big.sum() == 4 and (n == 1 or not big[:-4].any())
        if n > 1:  # mixed into longer rows: a planted row also holds ordinary elements
            assert all(np.isin(row, v).sum() <= 3 for row in X)


@pytest.mark.parametrize("name", ox.ALL)
def test_longdouble_restatement_against_mpmath(name):
    """A row's long-double value is a sum of n terms each good to a few units of 2^-64 of its size, on rows whose terms do
    not cancel: 2^-56 max(1, |f|) -- a sixteenth of the 2^-52 the device's bound starts at -- leaves room for n = 64 of
    them and for the rounding of 2 pi itself in long double.  The planted rows of the cos_2pi objectives, and rows of every
    objective from its own domain and from +-600."""
    pytest.importorskip("mpmath")
    todo = [(n, kind, slice(0, 4)) for n in (1, 7, 64) for kind in ("own", "wide")]
    if name in ox.COS_2PI:
        todo += [(1, "planted", slice(None)), (3, "planted", slice(None)), (64, "planted", slice(0, None, 5))]
    for n, kind, sl in todo:
        X = ox.rows(name, n, kind)[sl]
        got = ox.exact(name, X)
        for row, g in zip(X, got):
            want = ox.exact_mp(name, row)
            err = abs(float(g - np.longdouble(float(want))) - float(want - float(want)))  # (want's own double tail)
            assert err <= 2.0 ** -56 * max(1.0, abs(float(want))), (n, kind, row[:4], float(g), float(want))


@pytest.mark.parametrize("name,n,kind", CASES)
def test_numpy_stays_a_tenth_inside_the_projects_bar(name, n, kind):
    """numpy's own value is within 0.1 of 1e-13 max(1, |f|) + A of the exact one on every input (rows below 2^52): the
    reference of test_objectives_vs_oracle is good far beyond its bar, and E of the device's bound is small."""
    X = ox.rows(name, n, kind)
    X = X[~ox.huge_rows(X)]
    ref = ox.exact(name, X)
    err = np.abs(OBJECTIVES[name](X).astype(ox.LD) - ref).astype(np.float64)
    bar = 0.1 * (1.0e-13 * np.maximum(1.0, np.abs(ref.astype(np.float64))) + ox.argument_term(name, X))
    assert np.all(err <= bar), float(np.max(err / bar))


@pytest.mark.parametrize("name", ox.COSINE)
def test_nonfinite_elements_give_nan(name):
    for n in ox.NS:
        X = ox.nonfinite_rows(name, n)
        assert (~np.isfinite(X)).sum(axis=1).tolist() == [1] * len(X)
        with np.errstate(all="ignore"):
            assert np.isnan(OBJECTIVES[name](X)).all() and np.isnan(ox.exact(name, X).astype(np.float64)).all()


@pytest.mark.parametrize("name", ["quartic", "styblinski_tang"])
def test_kernel_association_is_not_numpys_power(name):
    """The kernels take x^4 as (x x)(x x), np.power(x, 4) is the correctly rounded power: the two differ in the last bit of
    about every second element, so these two objectives are held to the bound, not to numpy's bits -- and to the bits of the
    kernel's own association restated in numpy, which is as close to the exact value as numpy's."""
    for n in ox.NS:
        for kind in ("own", "wide"):
            X = ox.rows(name, n, kind)
            _, ratio, _ = ox.measure(name, X, ox.kernel_association(name, X))
            assert ratio.max() <= 1.0, (n, kind, ratio.max())
    X = ox.rows(name, 64, "own")
    assert not np.array_equal(ox.kernel_association(name, X), OBJECTIVES[name](X))
    assert np.mean((X * X) * (X * X) != np.power(X, 4)) > 0.25
