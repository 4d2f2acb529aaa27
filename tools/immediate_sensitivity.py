"""Does the oracle's own immediate-updating run hinge on the last bits of an objective value?  CPU only, oracle only.

A parity test of the ordered sweeps (tests/test_gpu_immediate_edges.py) means something only where it does not: the device's
cos / exp / sqrt may differ from numpy's in the last bits, and a `<=` decided by them would send the two runs apart for no
fault of the kernel.  Every case of the table (tests/_async_abi.py EDGE_CASES) is run once as is and three more times with
the objective replaced by f(X) * (1 + 2e-13 * h(row)), h in [-1, 1] a hash of the row's bytes and a salt -- keyed by the
point, not drawn from a stream: a rounding error is a function of the point, and equal points must keep equal values.
Per case: whether xall, nit and status came out unchanged bit for bit under all three salts, the largest deviation of xall
as a share of the search range and the largest relative deviation of funall.
usage: immediate_sensitivity.py [substring of a case id ...]"""
import os
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import oracle  # noqa: E402
from oracle.objectives import OBJECTIVES  # noqa: E402

import _async_abi  # noqa: E402

EPS = 2e-13
SALTS = (b"salt-1", b"salt-2", b"salt-3")
EXACT = {"rosenbrock", "sphere"}


def perturbed(f, salt):
    def g(X):
        X = np.ascontiguousarray(X, dtype=np.float64)
        X = X[None, :] if X.ndim == 1 else X
        h = np.array([zlib.crc32(row.tobytes() + salt) / float(0xFFFFFFFF) * 2.0 - 1.0 for row in X])
        return f(X) * (1.0 + EPS * h)

    return g


def main(argv):
    cases = [c for c in _async_abi.EDGE_CASES if not argv or any(w in _async_abi.case_id(c) for w in argv)]
    width = _async_abi.RANGE[1] - _async_abi.RANGE[0]
    print(f"oracle alone, rng=philox, seed {_async_abi.SEED}, bounds {list(_async_abi.RANGE)}, objective * (1 + {EPS:g} * h(row)), "
          f"{len(SALTS)} salts; W = {_async_abi.row_length(_async_abi.WIDE)}")
    print(f"{'case':<46} {'nit':>3} {'status':>6}  {'xall':>9} {'nit/status':>10}  {'max |dxall| / range':>19}  {'max rel dfunall':>15}")
    unstable = []
    for case in cases:
        method, objective, bounds, opts = _async_abi.case_options(case)
        base = oracle.minimize(objective, bounds, method=method, options=dict(opts), rng="philox")
        same_x, same_s, dx, df = True, True, 0.0, 0.0
        for salt in SALTS:
            run = oracle.minimize(perturbed(OBJECTIVES[objective], salt), bounds, method=method, options=dict(opts), rng="philox")
            same_s &= (run["nit"], run["status"]) == (base["nit"], base["status"])
            if run["xall"].shape != base["xall"].shape:
                same_x, dx, df = False, np.inf, np.inf
                continue
            same_x &= np.array_equal(run["xall"], base["xall"])
            dx = max(dx, float(np.abs(run["xall"] - base["xall"]).max()) / width)
            df = max(df, float((np.abs(run["funall"] - base["funall"]) / np.abs(base["funall"])).max()))
        tag = _async_abi.case_id(case)
        print(f"{tag:<46} {base['nit']:>3} {base['status']:>6}  {'same' if same_x else 'DIFFERS':>9} "
              f"{'same' if same_s else 'DIFFERS':>10}  {dx:>19.3g}  {df:>15.3g}", flush=True)
        # what the parity test needs: bit-stable without Shrink; with Shrink and an objective whose device value may differ in
        # the last bits, xall stable to 1e-14 of the range.  (sphere and rosenbrock are + - * only: the device returns numpy's
        # bits, no perturbation happens there, and the row is for information.)
        shrink = case[5].get("constraints") == "Shrink"
        if objective in EXACT:
            continue
        if (not same_s) or (not shrink and not same_x) or (shrink and dx > 1e-14):
            unstable.append(tag)
    print("needed: without Shrink, xall / nit / status the same; with Shrink, max |dxall| / range <= 1e-14.  sphere and rosenbrock "
          "rows are for information\n(+ - * only: the device returns numpy's bits, nothing is perturbed there) -- a Shrink run "
          "on them may well hang on last bits: a particle held at a wall moves by a few ulp, or not at all.")
    print("cases the parity test may not keep: " + (", ".join(unstable) if unstable else "none"))
    return 1 if unstable else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
