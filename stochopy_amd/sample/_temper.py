"""Parallel tempering (replica exchange) for ``method="mcmc"``: ladders of device-resident chains
(csrc/sx_sample_temper.hip; around a caller's own objective: csrc/sx_sample_unfused.hip).  The checks need no device."""
import ctypes as C

import numpy as np

from .. import _device, _lib
from ._chains import chain_args
from ._helpers import SampleResult


def check_ladder(temperatures, swap_every, rng):
    """(temperatures as float64 (K,), swap_every as int) of a tempered run, or the refusal: every message names
    ``temperatures``; nothing here touches the device."""
    if temperatures is None:
        raise ValueError("swap_every sets how often the rungs of a ladder exchange: it goes with temperatures=...")
    if isinstance(temperatures, (str, bytes)) or np.ndim(temperatures) == 0:
        raise TypeError("temperatures is a 1-D sequence of floats (1 = T_0 < T_1 < ...), not "
                        f"{type(temperatures).__name__}")
    try:
        T = np.array(temperatures, dtype=np.float64)
    except (TypeError, ValueError) as e:
        raise TypeError(f"temperatures is a 1-D sequence of floats: {e}") from None
    if T.ndim != 1 or T.size < 2:
        raise ValueError("temperatures is a 1-D sequence of K >= 2 floats")
    if not np.all(np.isfinite(T)) or T[0] != 1.0 or not np.all(np.diff(T) > 0.0):
        raise ValueError("temperatures are finite, start at temperatures[0] == 1.0 and increase strictly")
    if swap_every is None:
        swap_every = 1
    if isinstance(swap_every, bool) or not isinstance(swap_every, (int, np.integer)):
        raise TypeError(f"swap_every (the samples between two exchanges of a run with temperatures) is an integer, not "
                        f"{type(swap_every).__name__}")
    if swap_every < 1:
        raise ValueError("swap_every (the samples between two exchanges of a run with temperatures) is >= 1")
    if rng != "philox":
        raise ValueError('temperatures need rng="philox": the replicas make their draws in the kernel, keyed by replica')
    return T, int(swap_every)


def check_rungs(T, ndim):
    """A ladder lives in one workgroup: K <= sx_sample_tempered_max_rungs(ndim) (a host function of the library)."""
    most = int(_lib.lib().sx_sample_tempered_max_rungs(ndim))
    if T.size > most:
        raise ValueError(f"temperatures: a ladder lives in one workgroup, which holds {most} rungs of {ndim} variables "
                         f"(sx_sample_tempered_max_rungs), not {T.size}")


def swap_attempts(K, maxiter, swap_every):
    """(K - 1,) exchange events the pair (k, k + 1) takes part in: events j = 1 .. (maxiter - 1) // swap_every, the odd ones
    for even k, the even ones for odd k."""
    J = (maxiter - 1) // swap_every
    return np.array([(J + 1) // 2 if k % 2 == 0 else J // 2 for k in range(K - 1)], dtype=np.int64)


def run(s):
    L = _lib.lib()
    Cn, n, m = s.chains, s.ndim, s.maxiter
    T, every = s.temperatures, s.swap_every
    K = T.size
    R = Cn * K  # replicas: q = c * K + k is rung k of ladder c
    beta = 1.0 / T
    x0 = s.x0
    if x0 is not None and x0.ndim == 2:
        x0 = np.ascontiguousarray(np.repeat(x0, K, axis=0))  # one point per ladder, shared by its rungs
    ctx = _device.Context()
    t = _device.torch()
    with t.cuda.stream(ctx.stream):
        on_device_all = s.return_all and s.callback is None
        # (s is an mcmc Setup: method mcmc; nleap, jac and fd_step, which the kernels do not read, at their defaults)
        dev, a = chain_args(ctx, s, m if on_device_all else None, chains=R, x0=x0)
        nswap = ctx.zeros((R,), dtype=t.int64)
        dbeta = ctx.upload(beta)
        ptr = _device.ptr

        def cold(name):
            return dev[name].cpu().numpy().reshape((Cn, K) + tuple(dev[name].shape[1:]))[:, 0]

        if s.external is not None:
            prop = ctx.empty((R, n))

            def advance(i, steps):
                for it in range(i, i + steps):
                    _lib.check(L.sx_sample_propose(C.byref(a), it, ptr(prop), None, None, ctx.stream_ptr), "sx_sample_propose")
                    f = s.external(ctx, prop)
                    event = it >= 1 and it % every == 0
                    j = it // every
                    _lib.check(L.sx_sample_decide_tempered(C.byref(a), it, ptr(prop), ptr(f), ptr(dbeta), K,
                                                           int(not (event and j % 2 == 1)), ctx.stream_ptr),
                               "sx_sample_decide_tempered")
                    if event:
                        _lib.check(L.sx_sample_swap(C.byref(a), it, j, ptr(dbeta), K, ptr(nswap), ctx.stream_ptr),
                                   "sx_sample_swap")
        else:
            def advance(i, steps):  # one launch
                _lib.check(L.sx_sample_tempered_run(C.byref(a), ptr(dbeta), K, every, ptr(nswap), i, steps, ctx.stream_ptr),
                           "sx_sample_tempered_run")

        if s.callback is None:
            advance(0, m)
            xall = dev["xall"].cpu().numpy() if on_device_all else None
            funall = dev["funall"].cpu().numpy() if on_device_all else None
        else:
            # one launch per sample; the state the callback sees is stochopy_amd.sample's, of the COLD rungs
            xall = np.empty((Cn, m, n))
            funall = np.empty((Cn, m))
            for i in range(m):
                advance(i, 1)
                xall[:, i] = cold("cur")
                funall[:, i] = cold("fcur")
                facc_now, xbest_now = cold("facc"), cold("xbest")
                facc_now = np.where(cold("iacc") == 0, funall[:, 0], facc_now)  # (the first sample while there is none)
                b = int(np.argmin(facc_now))
                state = SampleResult(x=xbest_now[b], fun=facc_now[b], nit=i + 1,
                                     accept_ratio=1.0 if i == 0 else int(cold("nacc").sum()) / (Cn * (i + 1)))
                if s.return_all:
                    upto = max(i, 1)
                    state.update({"xall": xall[0, :upto] if Cn == 1 else xall[:, :upto],
                                  "funall": funall[0, :upto] if Cn == 1 else funall[:, :upto]})
                s.callback(xall[0, i] if Cn == 1 else xall[:, i], state)
        ctx.sync()
        nacc = dev["nacc"].cpu().numpy().reshape(Cn, K)
        nfeas = dev["nfeas"].cpu().numpy().reshape(Cn, K)
        swaps = nswap.cpu().numpy().reshape(Cn, K)[:, :K - 1]
        fbest, xbest = cold("facc"), cold("xbest")
    b = int(np.argmin(fbest))
    res = SampleResult(x=xbest[b], fun=fbest[b], nit=m, accept_ratio=int(nacc[:, 0].sum()) / (Cn * m))
    if s.reject:
        res["nreject"] = Cn * (m - 1) - int(nfeas[:, 0].sum())  # cold proposals that left the box
    res["accept_ratios"] = nacc / m
    res["temperatures"] = T.copy()
    attempts = swap_attempts(K, m, every)
    res["swap_ratios"] = np.where(attempts > 0, swaps / np.maximum(attempts, 1), 0.0)
    if s.return_all:
        res["xall"] = xall[0] if Cn == 1 else xall
        res["funall"] = funall[0] if Cn == 1 else funall
    return res
