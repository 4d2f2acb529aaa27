"""Per-chain step-size adaptation in a warm-up, burn-in and thinning (options ``warmup``, ``target_accept``, ``burn``,
``thin`` of ``sample.mcmc`` / ``sample.hmc``; csrc/sx_sample.hpp ``adapt_update``) and per-axis scale adaptation in that
warm-up (``metric="diag"``; csrc/sx_sample.hpp ``metric_update``).  The checks need no device."""
import numpy as np

OPTIONS = ("warmup", "target_accept", "burn", "thin")


class Adapt:
    """The checked options of one run: ``warmup`` W, ``target`` (the acceptance the rule steers to), ``burn`` B, ``thin`` T
    and ``rows`` M = ceil((maxiter - B) / T), the rows of xall / funall per chain."""

    windows = None  # metric="diag": (start, ends) of metric_windows(warmup); None without per-axis scales

    def __init__(self, warmup, target, burn, thin, maxiter):
        self.warmup, self.target, self.burn, self.thin = warmup, target, burn, thin
        self.rows = -(-(maxiter - burn) // thin)
        self.recorded = np.arange(burn, maxiter, thin)  # the samples xall / funall hold


def _integer(name, value):
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)):
        raise TypeError(f"{name} is an integer, not {type(value).__name__}")
    return int(value)


def _is(value, default):
    return not isinstance(value, bool) and isinstance(value, (int, np.integer)) and value == default


def given(warmup, target_accept, burn, thin):
    """The names of the options that are not at their defaults (``warmup=0, target_accept=None, burn=None, thin=1``)."""
    at_default = {"warmup": _is(warmup, 0), "target_accept": target_accept is None, "burn": burn is None, "thin": _is(thin, 1)}
    return [name for name in OPTIONS if not at_default[name]]


def refuse_with_temperatures(warmup, target_accept, burn, thin):
    names = given(warmup, target_accept, burn, thin)
    if names:
        raise ValueError(f"{' / '.join(names)}: not served together with temperatures (the tempered kernels neither adapt "
                         "their step nor thin what they record)")


def check(warmup, target_accept, burn, thin, rng, maxiter, default_target, metric=None):
    """None when every option is at its default (the run then takes the plain path), else the checked ``Adapt`` -- with
    ``metric="diag"`` carrying its windows.  Every message names its option; nothing here touches the device."""
    names = given(warmup, target_accept, burn, thin) + (["metric"] if metric is not None else [])
    if not names:
        return None
    warmup = _integer("warmup", warmup)
    thin = _integer("thin", thin)
    if burn is not None:
        burn = _integer("burn", burn)
    if target_accept is not None:
        if isinstance(target_accept, bool) or not isinstance(target_accept, (int, float, np.integer, np.floating)):
            raise TypeError(f"target_accept is a float in (0, 1), not {type(target_accept).__name__}")
        target_accept = float(target_accept)
    if not 0 <= warmup <= maxiter - 1:
        raise ValueError(f"warmup is an integer in [0, maxiter - 1] = [0, {maxiter - 1}], not {warmup}")
    if target_accept is not None:
        if warmup == 0:
            raise ValueError("target_accept is what the warm-up steers the acceptance to: it goes with warmup > 0")
        if not 0.0 < target_accept < 1.0:  # (a NaN fails both)
            raise ValueError(f"target_accept is a float in (0, 1), not {target_accept}")
    if burn is None:
        burn = warmup
    if not 0 <= burn <= maxiter - 1:
        raise ValueError(f"burn is an integer in [0, maxiter - 1] = [0, {maxiter - 1}], not {burn}")
    if thin < 1:
        raise ValueError(f"thin is an integer >= 1, not {thin}")
    check_metric(metric)
    if rng != "philox":
        raise ValueError(f'{" / ".join(names)} need rng="philox": the adapting and thinning kernels make their draws themselves')
    adapt = Adapt(warmup, default_target if target_accept is None else target_accept, burn, thin, maxiter)
    if metric is not None:
        if warmup < METRIC_MIN_WARMUP:
            raise ValueError(f'metric="diag" learns the scales in the warm-up: it needs warmup >= {METRIC_MIN_WARMUP}, not {warmup}')
        adapt.windows = metric_windows(warmup)
    return adapt


METRIC_MIN_WARMUP = 20
METRIC_MAX_WINDOWS = 8  # (sx_sample_metric.win_end; the schedule below makes at most 4)


def metric_windows(warmup):
    """``(start, ends)``: the windows (start, ends[0]], (ends[0], ends[1]], ... of a warm-up of ``warmup >= 20`` samples in
    which the per-axis scales are learnt.  The first 15 % of the warm-up settle the step size alone and the last 10 % settle
    it for the final scales; between them J doubling windows, J the largest of 4 ... 1 whose first window has 8 samples or
    more, the last one stretched to the end.  warmup 1000: 150 and (200, 300, 500, 900)."""
    start = (15 * warmup) // 100
    end = warmup - (10 * warmup) // 100
    span = end - start
    J = next(j for j in (4, 3, 2, 1) if span // (2 ** j - 1) >= 8)
    first = span // (2 ** J - 1)
    ends = [start + first * (2 ** j - 1) for j in range(1, J + 1)]
    ends[-1] = end
    return start, tuple(ends)


def check_metric(metric, with_temperatures=False):
    """``metric=None | "diag"``, after the other options' own checks; every message names ``metric``."""
    if metric is None:
        return
    if not isinstance(metric, str):
        raise TypeError(f'metric is None or "diag", not {type(metric).__name__}')
    if metric != "diag":
        raise ValueError(f'unknown metric {metric!r}: None or "diag" (per-axis scales learnt in the warm-up)')
    if with_temperatures:
        raise ValueError("metric: not served together with temperatures (the tempered kernels do not adapt)")
