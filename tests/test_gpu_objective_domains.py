"""sx_eval's seven objectives on their own domains, on +-600, and -- the two whose terms go through the hand-written cos_2pi
(csrc/sx_device.hpp) -- at signed zeros, integers, half and quarter integers up to 600 with their neighbours one ulp away,
the tiniest numbers and doubles beyond 2^52; against a long-double evaluation (tests/_objective_exact.py, itself held to
mpmath by tests/test_objective_exact_host.py).

The bound is measured against that reference, per case, not against the kernel: with E = max |numpy - exact| /
max(1, |exact|) over the case's rows, |device - exact| <= 4 max(E, 2^-52) max(1, |exact|) + A, A being the argument-rounding
term cos_2pi documents (10 n |2 pi x|max 2^-52 for rastrigin, e |2 pi x|max 2^-52 for ackley, 0 elsewhere).  Every test
prints `objective n kind E ratio` -- the device's largest error as a fraction of its bound -- before it asserts
(profiles/objective_domains.txt)."""
import numpy as np
import pytest

import _objective_exact as ox
from oracle.objectives import OBJECTIVES

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not ox.have_longdouble(),
                                 reason="np.longdouble has fewer than 63 mantissa bits here: no reference finer than double")]

CASES = [(name, n, kind) for name in ox.ALL for n in ox.NS for kind in ox.kinds(name)]


@pytest.fixture(scope="module")
def sa():
    import stochopy_amd

    return stochopy_amd


@pytest.mark.parametrize("name,n,kind", CASES)
def test_objective_within_the_measured_bound(sa, name, n, kind):
    X = ox.rows(name, n, kind)
    got = getattr(sa.factory, name)(X)
    E, ratio, ref = ox.measure(name, X, got)
    print("objective_domains %-16s n=%-4d %-8s rows=%-4d E=%.3e ratio=%.4f" % (name, n, kind, len(X), E, float(ratio.max())))
    assert np.all(np.isfinite(got))
    worst = int(np.argmax(ratio))
    assert ratio.max() <= 1.0, (worst, X[worst][:4], float(got[worst]), float(ref[worst]))
    if name in ox.BIT_EQUAL:
        assert np.array_equal(got, OBJECTIVES[name](X))
    if name in ("quartic", "styblinski_tang"):  # x^4 as (x x)(x x), not np.power: test_kernel_association_is_not_numpys_power
        assert np.array_equal(got, ox.kernel_association(name, X))
    if kind == "planted" and n == 1 and name == "rastrigin":
        # integers and half integers up to 600: the reduction leaves r = 0, the cosine is exactly +-1, x^2 -+ 10 is exact
        x = X[np.abs(X[:, 0]) <= 601.0, 0]
        f = got[np.abs(X[:, 0]) <= 601.0]
        whole, half = x == np.rint(x), np.abs(x - np.rint(x)) == 0.5
        assert whole.sum() >= 30 and half.sum() >= 60
        assert np.array_equal(f[whole], x[whole] ** 2)
        assert np.array_equal(f[half], 20.0 + x[half] ** 2)


@pytest.mark.parametrize("name", ox.COSINE)
def test_nonfinite_element_gives_nan(sa, name):
    for n in ox.NS:
        got = getattr(sa.factory, name)(ox.nonfinite_rows(name, n))
        assert np.isnan(got).all(), (n, got)
