// Device helpers the sampler kernels share: the resident chain kernels (sx_sample.hip) and the kernels around a
// caller-supplied objective (sx_sample_unfused.hip) compile the SAME expressions from here -- with bit-identical objective
// (and gradient) values the two paths give the same run, bit for bit.
#pragma once
#include "sx_rowops.hpp"

namespace sx {
namespace {

template <int LPR>
__device__ __forceinline__ double row_prod(double v) {
#pragma unroll
    for (int off = 1; off < LPR; off <<= 1) v *= __shfl_xor(v, off, kWave);
    return v;
}
template <int LPR>
__device__ __forceinline__ bool row_all(bool v) {
    return row_min<LPR>(v ? 1.0 : 0.0) != 0.0;
}

// Standard normals of a row, in the row kernels' element layout (sx_device.hpp philox_u53, as cma_normals_kernel): element
// e = LPR q + l belongs to call slot = (q >> 1) LPR + l and takes the cosine half (q even) or the sine half (q odd) of that
// call's Box-Muller pair.  Elements e0 (q even) and e0 + LPR therefore share one call, one logarithm, one square root and one
// angle -- and one lane: z0 / z1 are both of them.
template <int LPR>
__device__ __forceinline__ void philox_normal_pair(int e0, uint32_t chain, uint32_t gen, uint32_t purpose, uint32_t k0,
                                                   uint32_t k1, double &z0, double &z1) {
    const uint32_t slot = ((uint32_t)e0 / (2u * LPR)) * LPR + ((uint32_t)e0 & (LPR - 1u));
    const U4 w = philox4x32_10(slot, chain, gen, purpose, k0, k1);
    const double d0 = u53(w.x, w.y), d1 = u53(w.z, w.w);
    const double rad = sqrt(-2.0 * log(1.0 - d0));
    double sn, cs;
    sincos_mid(kTwoPi * d1, sn, cs);
    z0 = rad * cs;
    z1 = rad * sn;
}
__device__ __forceinline__ double philox_log_accept(uint32_t chain, uint32_t gen, uint32_t k0, uint32_t k1) {
    const U4 w = philox4x32_10(0u, chain, gen, kPurposeSampleAccept, k0, k1);
    return log(u53(w.x, w.y));
}

// the scalars of one chain (identical in every lane of its row group)
struct ChainState {
    double fcur, facc, fmin;
    int64_t iacc, imin, nacc, nfeas;
    __device__ __forceinline__ void load(const sx_sample_args &a, int64_t c) {
        fcur = a.fcur[c], facc = a.facc[c], fmin = a.fmin[c];
        iacc = a.iacc[c], imin = a.imin[c], nacc = a.nacc[c], nfeas = a.nfeas[c];
    }
    __device__ __forceinline__ void store(const sx_sample_args &a, int64_t c) const {
        a.fcur[c] = fcur, a.facc[c] = facc, a.fmin[c] = fmin;
        a.iacc[c] = iacc, a.imin[c] = imin, a.nacc[c] = nacc, a.nfeas[c] = nfeas;
    }
    __device__ __forceinline__ void start(double f0) {
        fcur = f0, facc = __builtin_huge_val(), fmin = f0;
        iacc = 0, imin = 0, nacc = 0, nfeas = 0;
    }
    // an accepted sample `it` of value f: mcmc/_mcmc.py:131-134, hmc/_hmc.py:167-172 (best ACCEPTED sample, plain <) and
    // numpy's argmin over funall (hmc/_hmc.py:187: the first NaN wins, else the first minimum).  Returns which changed.
    __device__ __forceinline__ void accept(double f, int64_t it, bool &acc_best, bool &arg_best) {
        fcur = f;
        nacc += 1;
        acc_best = f < facc;
        if (acc_best) facc = f, iacc = it;
        arg_best = best_before(f, fmin);
        if (arg_best) fmin = f, imin = it;
    }
};

// the initial sample (mcmc/_mcmc.py:93, hmc/_hmc.py:124): the given x0, or uniform(lower, upper) = lower + (upper - lower) * u
template <int LPR>
__device__ __forceinline__ double initial_value(const sx_sample_args &a, int64_t c, int e) {
    if (a.x0 != nullptr) return a.x0[c * a.x0_stride + e];
    const double lo = a.lower[e];
    return lo + (a.upper[e] - lo) * philox_u53(e, LPR, (uint32_t)c, 0u, kPurposeSampleInit, a.key0, a.key1);
}

template <int LPR>
__device__ __forceinline__ bool row_in_box(const sx_sample_args &a, const double *U, int n, int l) {
    bool in = true;
    for (int e = l; e < n; e += LPR) {
        const double v = U[e];
        in = in && v >= a.lower[e] && v <= a.upper[e];
    }
    return row_all<LPR>(in);
}

}  // namespace
}  // namespace sx
