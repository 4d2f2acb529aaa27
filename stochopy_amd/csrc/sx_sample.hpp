// Device helpers the sampler kernels share: the resident chain kernels (sx_sample.hip) and the kernels around a
// caller-supplied objective (sx_sample_unfused.hip) compile the SAME expressions from here -- with bit-identical objective
// (and gradient) values the two paths give the same run, bit for bit.  The tempered ladders (sx_sample_temper.hip, and their
// decide / swap kernels in sx_sample_unfused.hip) share them too, with the exchange rule at the end of this file.
#pragma once
#include <type_traits>

#include "sx_host.hpp"
#include "sx_rowops.hpp"

namespace sx {
namespace {

enum { kMcmc = 0, kHmcFd = 1, kHmcAnalytic = 2 };  // kernel variants

// doubles of LDS one chain needs (the resident kernels: sx_sample.hip, sx_sample_temper.hip)
__host__ __device__ inline int sample_row_doubles(int variant, int n) {
    const int S = gen_row_stride(n);
    return variant == kMcmc ? n + S : variant == kHmcAnalytic ? 2 * n + S : 2 * n + 3 * S;
}
// waves per workgroup: the largest power of two with <= 16 chains and <= 64 KiB of LDS; one wave may need more than that
// (hmc with finite differences on rows of ~2 048 elements: the launch then raises the kernel's dynamic-LDS limit)
inline int sample_waves(int variant, int n) {
    const int rpw = kWave / lanes_per_row(n);
    const int fit = (64 * 1024) / (8 * sample_row_doubles(variant, n) * rpw);
    int w = 1;
    while (2 * w <= fit && 2 * w * rpw <= kMaxRowsPerBlock && 2 * w <= kMaxWavesPerBlock) w *= 2;
    return w;
}

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
    // parallel tempering: a state of value f ARRIVES by an exchange at sample `it` -- compared as an accepted sample is, but an
    // exchange is no proposal (nacc and nfeas stay)
    __device__ __forceinline__ void arrive(double f, int64_t it, bool &acc_best) {
        fcur = f;
        acc_best = f < facc;
        if (acc_best) facc = f, iacc = it;
        if (best_before(f, fmin)) fmin = f, imin = it;
    }
};

// Step-size adaptation in a warm-up (sx_sample_adapt; dual averaging, Hoffman & Gelman 2014, on a per-chain MULTIPLIER of
// a.step): the constants of the rule.  They are fixed, not options.
constexpr double kAdaptT0 = 10.0;                  // eta = 1 / (t + t0): the early samples count less
constexpr double kAdaptGamma = 0.05;               // logs = mu - (sqrt(t) / gamma) * hbar
constexpr double kAdaptLogMu = 2.302585092994046;  // mu = log(10): the multiplier is drawn towards 10 x its start, 1.0
// (the averaging weight t^(-kappa), kappa = 3/4, is formed as 1 / (sqrt(t) * sqrt(sqrt(t))): no pow)

// the adaptation scalars of one chain (identical in every lane of its row group), carried like ChainState.  With warmup == 0
// nothing adapts and the arrays may be NULL: s stays 1.0 and 1.0 * step is step, bit for bit.
struct AdaptState {
    double s, hbar, logsbar;  // the multiplier in use, the averaged (target - alpha), the averaged log multiplier
    int64_t nacc_warm;        // nacc after sample `warmup`
    __device__ __forceinline__ void load(const sx_sample_adapt &ad, int64_t c) {
        start();
        if (ad.warmup > 0) s = ad.scale[c], hbar = ad.hbar[c], logsbar = ad.logsbar[c], nacc_warm = ad.nacc_warm[c];
    }
    __device__ __forceinline__ void store(const sx_sample_adapt &ad, int64_t c) const {
        if (ad.warmup > 0) ad.scale[c] = s, ad.hbar[c] = hbar, ad.logsbar[c] = logsbar, ad.nacc_warm[c] = nacc_warm;
    }
    __device__ __forceinline__ void start() { s = 1.0, hbar = 0.0, logsbar = 0.0, nacc_warm = 0; }
};

// the adapting kernels' last argument; the plain kernels take an empty struct in its place, which they never read
struct NoAdapt {};
template <bool ADAPT>
using AdaptArg = std::conditional_t<ADAPT, sx_sample_adapt, NoAdapt>;

// After the decision of sample `it` >= 1 (d its own log acceptance ratio; feasible: it passed the box test; nacc the count
// with this sample): one step of the rule for it <= warmup, the averaged multiplier frozen at it == warmup.  The decision
// itself accepts a NaN d; HERE a NaN d counts as alpha = 0, so that a diverged trajectory shrinks the step.
__device__ __forceinline__ void adapt_update(AdaptState &ad, int64_t warmup, double target, int64_t it, bool feasible, double d,
                                             int64_t nacc) {
    if (it > warmup) return;
    const double t = (double)it;
    const double alpha = !feasible ? 0.0 : d < 0.0 ? exp(d) : d >= 0.0 ? 1.0 : 0.0;
    const double eta = 1.0 / (t + kAdaptT0);
    ad.hbar = (1.0 - eta) * ad.hbar + eta * (target - alpha);
    const double rt = sqrt(t);
    const double logs = kAdaptLogMu - (rt / kAdaptGamma) * ad.hbar;
    const double w = 1.0 / (rt * sqrt(rt));
    ad.logsbar = w * logs + (1.0 - w) * ad.logsbar;
    ad.s = it < warmup ? exp(logs) : exp(ad.logsbar);
    if (it == warmup) ad.nacc_warm = nacc;
}
// thinning: is sample `it` recorded, and in which row of xall / funall (rec_every < 2^31, it < maxiter < 2^31)
__device__ __forceinline__ bool adapt_record(const sx_sample_adapt &ad, int64_t it, int64_t &row) {
    if (it < ad.rec_start) return false;
    const uint32_t off = (uint32_t)(it - ad.rec_start), every = (uint32_t)ad.rec_every;
    row = (int64_t)(off / every);
    return off % every == 0u;
}

// what every *_adapt entry point requires of `ad` next to its own checks of `a` (which come first: a is not null here)
inline int check_adapt(const sx_sample_args *a, const sx_sample_adapt *ad) {
    SX_REQUIRE(ad != nullptr, "sx_sample (adapt): null adaptation args");
    SX_REQUIRE(a->rng == SX_RNG_PHILOX, "sx_sample (adapt): the draws are made in the kernels (SX_RNG_PHILOX)");
    SX_REQUIRE(ad->warmup >= 0 && ad->warmup <= a->maxiter - 1, "sx_sample (adapt): warmup outside [0, maxiter - 1]");
    SX_REQUIRE(ad->rec_start >= 0 && ad->rec_start <= a->maxiter - 1, "sx_sample (adapt): rec_start outside [0, maxiter - 1]");
    SX_REQUIRE(ad->rec_every >= 1 && ad->rec_every < (int64_t)1 << 31, "sx_sample (adapt): rec_every outside [1, 2^31)");
    SX_REQUIRE(ad->rec_rows == (a->maxiter - ad->rec_start + ad->rec_every - 1) / ad->rec_every,
               "sx_sample (adapt): rec_rows is not ceil((maxiter - rec_start) / rec_every)");
    if (ad->warmup > 0) {
        SX_REQUIRE(ad->scale && ad->hbar && ad->logsbar && ad->nacc_warm, "sx_sample (adapt): null adaptation state pointer");
        SX_REQUIRE(ad->target > 0.0 && ad->target < 1.0, "sx_sample (adapt): target outside (0, 1)");
    }
    return 0;
}

// the resident kernels walk the recorded samples instead: the first one at or after it0 and its row, then + rec_every / + 1
__device__ __forceinline__ void adapt_first_record(const sx_sample_adapt &ad, int64_t it0, int64_t &next, int64_t &row) {
    next = ad.rec_start, row = 0;
    if (it0 > ad.rec_start) {
        row = (it0 - ad.rec_start + ad.rec_every - 1) / ad.rec_every;
        next = ad.rec_start + row * ad.rec_every;
    }
}

// parallel tempering, the exchange of rungs (kl, kl + 1) of a ladder after sample `it`: both replicas exchange their states when
// this holds.  fl / fu their current values, bl / bu their inverse temperatures, ql the LOWER rung's replica index.
__device__ __forceinline__ bool tempered_swap(double fl, double fu, double bl, double bu, uint32_t ql, uint32_t it, uint32_t k0,
                                              uint32_t k1) {
    const U4 w = philox4x32_10(0u, ql, it, kPurposeSampleSwap, k0, k1);
    const double d = (bl - bu) * (fl - fu);
    return (d < 0.0 ? d : 0.0) > log(u53(w.x, w.y));  // (a NaN d exchanges, as a NaN d accepts)
}
// the lower rung of the pair rung `rung` belongs to at exchange event j (odd j: (0,1), (2,3), ...; even j: (1,2), (3,4), ...),
// or -1 when the rung sits this event out
__device__ __forceinline__ int tempered_pair(int rung, int K, int64_t j) {
    const int kl = (rung & 1) == (int)((j + 1) & 1) ? rung : rung - 1;
    return kl >= 0 && kl + 1 < K ? kl : -1;
}

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
