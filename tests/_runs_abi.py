"""What the helpers of the four batched-runs kernels share (tests/_de_runs_abi.py, _pso_runs_abi.py, _cma_runs_abi.py,
_vd_runs_abi.py).  A plain helper module (imported, not collected)."""

FILL = -12345.678  # no run produces it: an element the kernel does not write cannot pass for a result


def largest(fits, lo, hi):
    """The largest k in [lo, hi) with fits(k), fits being true up to some point and false beyond."""
    assert fits(lo) and not fits(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if fits(mid):
            lo = mid
        else:
            hi = mid
    return lo


def launch_filled(batch, fills):
    """Fill the named output tensors of a production batch (optimize/_runs.py Batch) with `fills`, launch it, return its
    outputs as numpy arrays by name."""
    with batch.stream():
        for name, value in fills.items():
            batch.dev[name].fill_(value)
    batch.launch()
    return batch.fetch()
