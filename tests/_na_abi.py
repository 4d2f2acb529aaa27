"""The Neighbourhood Algorithm's cell-walk kernels (csrc/sx_na.hip) for the tests: one generation of walks driven through
the C ABI on a model store the test made up -- sx_na_begin, per free axis sx_na_axis with the host's scalar d1 recurrence
in between (as optimize/_na.py writes it), sx_na_commit -- with the padding of the store and of the cell distances
filled by the caller, so that a read or a write past the models shows.  A plain helper module (imported, not collected)."""

import numpy as np

WS_BLOCKS = 64  # optimize/_na.py sizes the workspace of the wall partials for the cap of sx_na_blocks: 2 * P * 64 doubles


def _padding(pad, shape):
    """pad: a value, or a callable shape -> array (fresh numbers for every buffer)."""
    return np.array(pad(shape), dtype=np.float64) if callable(pad) else np.full(shape, pad, dtype=np.float64)


def blocks(M):
    """sx_na_blocks as its contract states it: one workgroup per 256 models, 64 at the most."""
    return min(-(-M // 256), 64)


def walks(models, cap, kidx, u, free, pad):
    """One generation: walk i starts at model kidx[i] and draws with u[i] along every free axis.  models (M, n) go
    column-major into an (n, cap) store, cap > M + P; store columns >= M and every cell distance start as `pad`.
    Returns a dict: X (P, n) after sx_na_commit; XT0 / d20, the buffers as uploaded; d2_begin, the cell distances
    right after sx_na_begin; XT / d2, the buffers at the end."""
    from stochopy_amd import _device, _lib

    models = np.asarray(models, dtype=np.float64)
    M, n = models.shape
    kidx = np.asarray(kidx, dtype=np.int64)
    P = len(kidx)
    u = np.ascontiguousarray(u, dtype=np.float64)
    free = np.asarray(free, dtype=bool)
    assert cap > M + P and u.shape == (P, n) and free.shape == (n,) and kidx.min() >= 0 and kidx.max() < M
    XT0 = _padding(pad, (n, cap))
    XT0[:, :M] = models.T
    d20 = _padding(pad, (P, cap))
    ctx = _device.Context()
    L, ptr, t, sp = ctx.L, _device.ptr, _device.torch(), ctx.stream_ptr
    with t.cuda.stream(ctx.stream):
        d_XT, d_d2, d_kidx, d_u = ctx.upload(XT0), ctx.upload(d20), ctx.upload(kidx), ctx.upload(u)
        d_fixed = ctx.upload((~free).astype(np.int32))
        d_X = ctx.upload(np.full((P, n), np.nan))
        d_d1, d_xnew = ctx.empty((P,)), ctx.upload(np.full(P, np.nan))
        d_ws = ctx.upload(np.full(2 * P * WS_BLOCKS, np.nan))
        _lib.check(L.sx_na_begin(ptr(d_XT), cap, M, n, ptr(d_kidx), P, ptr(d_X), ptr(d_d2), sp), "sx_na_begin")
        d2_begin = d_d2.cpu().numpy()
        centre = models[kidx]
        d1 = [0.0] * P
        jp = -1
        for j in np.flatnonzero(free).tolist():
            d_d1.copy_(t.from_numpy(np.array(d1, dtype=np.float64)))
            _lib.check(L.sx_na_axis(ptr(d_XT), cap, M, n, j, jp, ptr(d_kidx), P, ptr(d_u), ptr(d_d1), ptr(d_X),
                                    ptr(d_d2), ptr(d_ws), ptr(d_xnew), sp), "sx_na_axis")
            jp = j
            if j < n - 1:
                xnew = d_xnew.cpu().numpy()
                cj = centre[:, j]
                zero = np.float64(0.0)
                # numpy SCALAR arithmetic, as optimize/_na.py and the reference write it: `** 2` on a scalar is libm pow
                d1 = [d1[i] + ((cj[i] - xnew[i]) ** 2 - zero ** 2) for i in range(P)]
        _lib.check(L.sx_na_commit(ptr(d_X), P, n, ptr(d_fixed), ptr(d_XT), cap, M, sp), "sx_na_commit")
        out = dict(X=d_X.cpu().numpy(), XT=d_XT.cpu().numpy(), d2=d_d2.cpu().numpy())
    ctx.sync()
    out.update(XT0=XT0, d20=d20, d2_begin=d2_begin)
    return out


def uniforms(seed, gen, P, n):
    """sx_na_uniforms: the (P, n) block of generation `gen`, every element drawn (fixed axes too).  The buffer is 300
    doubles longer than the block and starts as NaN: the tail must come back untouched."""
    from stochopy_amd import _device, _lib, _rng

    ctx = _device.Context()
    t = _device.torch()
    key0, key1 = _rng.philox_key(seed)
    with t.cuda.stream(ctx.stream):
        d_u = ctx.upload(np.full(P * n + 300, np.nan))
        _lib.check(ctx.L.sx_na_uniforms(_device.ptr(d_u), P, n, gen, key0, key1, ctx.stream_ptr), "sx_na_uniforms")
        got = d_u.cpu().numpy()
    assert np.isnan(got[P * n:]).all(), "sx_na_uniforms wrote past P * n"
    return got[:P * n].reshape(P, n)
