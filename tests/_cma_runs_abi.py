"""The batched-runs CMA-ES kernel (csrc/sx_cma_runs.hip), the host side of its C ABI restated for the tests: the LDS layout
the kernel's header comment documents, in bytes.  A plain helper module (imported, not collected)."""

LDS_LIMIT = 160 * 1024
MAX_DIM = 32


def solver_size(n):
    """M2 of the one-workgroup Jacobi solver that serves dimension n."""
    return 16 if n <= 16 else 32


def lds_bytes(P, n):
    """C[n][ldn] | B[n][ldn] | nine vectors of n | lam, scl, inv [M2] each | fit[P] | order[P] as int32 | red[24] | part[8][4] |
    max(candidates P * (n + 8), Jacobi storage 4 * M2 * (M2 + 1) + 2 * M2), in bytes; ldn = n | 1."""
    ldn, m2 = n | 1, solver_size(n)
    fixed = 2 * n * ldn + 9 * n + 3 * m2 + P + (P + 1) // 2 + 24 + 32
    return 8 * (fixed + max(P * (n + 8), 4 * m2 * (m2 + 1) + 2 * m2))


def workspace_bytes(R, maxiter):
    """One zero-initialised best-fitness history of maxiter doubles per run."""
    return 8 * R * maxiter


def largest_popsize(lib, n):
    """The largest P with sx_cma_runs_lds_bytes(P, n) > 0, by bisection (the function refuses everything above it)."""
    lo, hi = 2, 1 << 20
    assert lib.sx_cma_runs_lds_bytes(lo, n) > 0 and lib.sx_cma_runs_lds_bytes(hi, n) < 0
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if lib.sx_cma_runs_lds_bytes(mid, n) > 0:
            lo = mid
        else:
            hi = mid
    return lo
