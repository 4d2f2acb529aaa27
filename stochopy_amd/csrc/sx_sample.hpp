// What the sampler kernels share, written once: the draws, a chain's scalars and its step-size adaptation, the STEP of a chain
// (the mcmc block perturbation and the Metropolis decision, for the kernels around a caller-supplied objective,
// sx_sample_unfused.hip, and the tempered ladders, sx_sample_temper.hip), the unfused tail, the exchange rule of the ladders,
// and the host's argument check and workgroup size.  The two resident kernels (sx_sample_kernels.hpp) share the draws, the scalars and
// the adaptation, but spell the step themselves (folded into the functions below it ran 1 - 3 % slower there: DESIGN.md 19);
// the same expressions under -ffp-contract=off -- with bit-identical objective (and gradient) values the resident and the
// unfused path give the same run, bit for bit, which tests/test_gpu_sample_batched.py holds them to.
#pragma once
#include <string>
#include <type_traits>

#include "sx_host.hpp"
#include "sx_rowops.hpp"

namespace sx {
namespace {

enum { kMcmc = 0, kHmcFd = 1, kHmcAnalytic = 2 };  // kernel variants

// doubles of LDS one chain needs (the resident kernels: sx_sample.hip, sx_sample_temper.hip); `metric`: with the chain's
// per-axis steps eff[n] behind them (sx_sample_metric)
__host__ __device__ inline int sample_row_doubles(int variant, int n, bool metric = false) {
    const int S = gen_row_stride(n);
    return (variant == kMcmc ? n + S : variant == kHmcAnalytic ? 2 * n + S : 2 * n + 3 * S) + (metric ? n : 0);
}
// Waves per workgroup of a kernel with one row group per chain (or row): the largest power of two within the row kernels' caps
// (kMaxWavesPerBlock waves, kMaxRowsPerBlock rows) whose rows, at `row_bytes` of LDS each, fit 64 KiB.  One wave may need more
// than that (hmc with finite differences on rows of ~2 048 elements: the launch then raises the kernel's dynamic-LDS limit).
inline int waves_per_workgroup(int n, size_t row_bytes) {
    const int rpw = kWave / lanes_per_row(n);
    int w = 1;
    while (2 * w <= kMaxWavesPerBlock && 2 * w * rpw <= kMaxRowsPerBlock && 2 * w * rpw * row_bytes <= 64 * 1024) w *= 2;
    return w;
}
inline int sample_waves(int variant, int n, bool metric = false) {
    return waves_per_workgroup(n, sizeof(double) * sample_row_doubles(variant, n, metric));
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

// the adapting kernels' last argument; the plain kernels take an empty struct in its place, which they never read.  The
// kernels with per-axis scales (METRIC, which implies ADAPT) take sx_sample_adapt with sx_sample_metric behind it.
struct NoAdapt {};
struct MetricAdapt : sx_sample_adapt {
    sx_sample_metric mt;
};
template <bool ADAPT, bool METRIC = false>
using AdaptArg = std::conditional_t<METRIC, MetricAdapt, std::conditional_t<ADAPT, sx_sample_adapt, NoAdapt>>;
template <bool ADAPT, bool METRIC = false>
AdaptArg<ADAPT, METRIC> adapt_arg(const sx_sample_adapt *ad, const sx_sample_metric *mt = nullptr) {
    if constexpr (METRIC) {
        MetricAdapt r;
        static_cast<sx_sample_adapt &>(r) = *ad;
        r.mt = *mt;
        return r;
    } else if constexpr (ADAPT) {
        return *ad;
    } else {  // (the plain entry points pass no `ad`)
        return {};
    }
}

// After the decision of sample `it` >= 1 (d its own log acceptance ratio; feasible: it passed the box test; nacc the count
// with this sample): one step of the rule for it <= warmup, the averaged multiplier frozen at it == warmup.  The decision
// itself accepts a NaN d; HERE a NaN d counts as alpha = 0, so that a diverged trajectory shrinks the step.
// RESTARTS (the kernels with per-axis scales): the rule's clock runs from `origin`, the last window end before `it`, and the
// multiplier is sbase times what the rule gives; without them origin = 0 and there is no sbase.
template <bool RESTARTS>
__device__ __forceinline__ void adapt_rule(AdaptState &ad, int64_t warmup, double target, int64_t it, int64_t origin, double sbase,
                                           bool feasible, double d, int64_t nacc) {
    if (it > warmup) return;
    const double t = RESTARTS ? (double)(it - origin) : (double)it;
    const double alpha = !feasible ? 0.0 : d < 0.0 ? exp(d) : d >= 0.0 ? 1.0 : 0.0;
    const double eta = 1.0 / (t + kAdaptT0);
    ad.hbar = (1.0 - eta) * ad.hbar + eta * (target - alpha);
    const double rt = sqrt(t);
    const double logs = kAdaptLogMu - (rt / kAdaptGamma) * ad.hbar;
    const double w = 1.0 / (rt * sqrt(rt));
    ad.logsbar = w * logs + (1.0 - w) * ad.logsbar;
    ad.s = it < warmup ? exp(logs) : exp(ad.logsbar);
    if constexpr (RESTARTS) ad.s = sbase * ad.s;
    if (it == warmup) ad.nacc_warm = nacc;
}
__device__ __forceinline__ void adapt_update(AdaptState &ad, int64_t warmup, double target, int64_t it, bool feasible, double d,
                                             int64_t nacc) {
    adapt_rule<false>(ad, warmup, target, it, 0, 1.0, feasible, d, nacc);
}

// ---------------------------------------------------------------------------------------------------------------------
// Per-axis scales in the warm-up (sx_sample_metric; include/stochopy_hip.h states the rule).  Chain c's m, mean and M2 are rows
// of (C, n) DEVICE arrays and its sbase an element of a (C) one: they are touched after a decision inside a window and at a
// window end only, every element by the lane that owns it, so they need neither LDS nor a fence.  What a sample reads per
// element is eff = m * step: the resident kernels keep it in the chain's LDS row, the unfused ones form it from m.
// ---------------------------------------------------------------------------------------------------------------------
constexpr double kMetricShrinkCount = 5.0;     // v = (N / (N + 5)) var + (5 / (N + 5)) 1e-3 h^2: Stan's shrinkage of a window's
constexpr double kMetricShrinkScale = 1.0e-3;  // variance towards 1e-3 of the squared half-width (the units `step` is in)

// where sample `it` stands among the windows: N = it - b_{j-1} inside window j (0 outside all), whether it ends it, and the
// origin of the rule's clock, the last end BEFORE it (0 when there is none).  Neither is stored: both follow from it.
struct MetricClock {
    int64_t N = 0, origin = 0;
    bool end = false;
};
__device__ __forceinline__ MetricClock metric_clock(const sx_sample_metric &mt, int64_t it) {
    MetricClock k;
    int64_t lo = mt.win_start;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        if (j < mt.nwin) {
            const int64_t hi = mt.win_end[j];
            if (it > lo && it <= hi) k.N = it - lo, k.end = it == hi;
            if (hi < it) k.origin = hi;
            lo = hi;
        }
    }
    return k;
}
// chain c's scalar beside AdaptState
__device__ __forceinline__ double metric_load_sbase(const sx_sample_metric &mt, int64_t c) { return mt.nwin > 0 ? mt.sbase[c] : 1.0; }
// element e of chain c's eff
__device__ __forceinline__ double metric_eff(const sx_sample_args &a, const sx_sample_metric &mt, int64_t c, int e) {
    return mt.nwin > 0 ? mt.m[c * a.n + e] * a.step[e] : 1.0 * a.step[e];
}
// sample 0: m = 1, the moments empty, sbase = 1 (`active`: a padding row group stores nothing, here and below)
template <int LPR>
__device__ __forceinline__ void metric_start(const sx_sample_args &a, const sx_sample_metric &mt, int64_t c, int l, bool active,
                                             double &sbase) {
    sbase = 1.0;
    if (mt.nwin == 0 || !active) return;
    for (int e = l; e < a.n; e += LPR) mt.m[c * a.n + e] = 1.0, mt.mean[c * a.n + e] = 0.0, mt.M2[c * a.n + e] = 0.0;
    if (l == 0) mt.sbase[c] = 1.0;
}
// After the decision of sample `it` >= 1, in the place of adapt_update: the Welford step on the chain's current state x(e), the
// dual averaging on its clock, and at a window end the new scales -- put(e, eff_e) takes them -- and the restart of the step
// size.  Every lane of the row group takes the same branches (the scalars are uniform in it, `ok` is reduced over it).
template <int LPR, class X, class Put>
__device__ __forceinline__ void metric_update(const sx_sample_args &a, const MetricAdapt &ad, AdaptState &as, double &sbase,
                                              int64_t c, int l, bool active, int64_t it, bool feasible, double d, int64_t nacc,
                                              X &&x, Put &&put) {
    if (it > ad.warmup) return;  // (every window lies inside the warm-up: the sampling phase pays this test alone)
    const sx_sample_metric &mt = ad.mt;
    const int n = a.n;
    const MetricClock k = metric_clock(mt, it);
    const double N = (double)k.N;
    if (k.N > 0) {
        for (int e = l; e < n; e += LPR) {
            const double v = x(e);
            const double mean0 = mt.mean[c * n + e];
            const double delta = v - mean0;
            const double mean = mean0 + delta / N;
            const double M2 = mt.M2[c * n + e] + delta * (v - mean);
            if (active) mt.mean[c * n + e] = mean, mt.M2[c * n + e] = M2;
        }
    }
    adapt_rule<true>(as, ad.warmup, ad.target, it, k.origin, sbase, feasible, d, nacc);
    if (!k.end) return;
    const double wn = N / (N + kMetricShrinkCount), wp = (kMetricShrinkCount / (N + kMetricShrinkCount)) * kMetricShrinkScale;
    const auto r_of = [&](int e) {
        const double h = 0.5 * (a.upper[e] - a.lower[e]);
        return sqrt(wn * (mt.M2[c * n + e] / (N - 1.0)) + wp * (h * h));
    };
    double sumlog = 0.0;
    bool ok = true;
    for (int e = l; e < n; e += LPR) {
        const double r = r_of(e);
        ok = ok && r > 0.0 && r < __builtin_huge_val();  // (a NaN fails both)
        sumlog += log(r);
    }
    ok = row_all<LPR>(ok);
    const double gm = exp(row_sum<LPR>(sumlog) / (double)n);
    for (int e = l; e < n; e += LPR) {
        if (ok) {
            const double m = r_of(e) / gm;
            put(e, m * a.step[e]);
            if (active) mt.m[c * n + e] = m;
        }
        if (active) mt.mean[c * n + e] = 0.0, mt.M2[c * n + e] = 0.0;
    }
    sbase = sbase * exp(as.logsbar);
    as.hbar = 0.0, as.logsbar = 0.0, as.s = sbase;
    if (active && l == 0) mt.sbase[c] = sbase;
}
// what every *_metric entry point requires of `mt` next to check_adapt (which comes first: ad is not null here)
inline int check_metric(const sx_sample_adapt *ad, const sx_sample_metric *mt) {
    SX_REQUIRE(mt != nullptr, "sx_sample (metric): null metric args");
    SX_REQUIRE(mt->nwin >= 0 && mt->nwin <= 8, "sx_sample (metric): nwin outside [0, 8]");
    if (mt->nwin > 0) {
        SX_REQUIRE(mt->sbase && mt->m && mt->mean && mt->M2, "sx_sample (metric): null metric state pointer");
        SX_REQUIRE(mt->win_start >= 0, "sx_sample (metric): win_start is negative");
        int64_t lo = mt->win_start;
        for (int j = 0; j < mt->nwin; lo = mt->win_end[j++])
            SX_REQUIRE(mt->win_end[j] > lo, "sx_sample (metric): the window ends do not increase from win_start");
        SX_REQUIRE(lo <= ad->warmup, "sx_sample (metric): a window ends after the warm-up");
    }
    return 0;
}
// thinning: is sample `it` recorded, and in which row of xall / funall (rec_every < 2^31, it < maxiter < 2^31)
__device__ __forceinline__ bool adapt_record(const sx_sample_adapt &ad, int64_t it, int64_t &row) {
    if (it < ad.rec_start) return false;
    const uint32_t off = (uint32_t)(it - ad.rec_start), every = (uint32_t)ad.rec_every;
    row = (int64_t)(off / every);
    return off % every == 0u;
}

// SX_REQUIRE with the message "<who>: <what>", `who` the entry point's name in scope (here and in the three .hip files)
#define SX_SAMPLE_REQUIRE(cond, what) SX_REQUIRE(cond, std::string(who) + ": " what)

// What every sampler entry point `who` requires of sx_sample_args before it launches samples [it0, it0 + steps).  `resident`:
// the objective is compiled into the kernel (fun_id names one, finite differences need their step here); `host_draws`: the
// kernel can read the reference's stream (the resident chain kernels alone).
inline int check_sample_args(const char *who, const sx_sample_args *a, int64_t it0, int64_t steps, bool resident, bool host_draws) {
    SX_SAMPLE_REQUIRE(a != nullptr, "null args");
    SX_SAMPLE_REQUIRE(a->cur && a->fcur && a->facc && a->fmin && a->xbest && a->iacc && a->imin && a->nacc && a->nfeas,
                      "null state pointer");
    SX_SAMPLE_REQUIRE(a->lower && a->upper && a->step, "bounds / step missing");
    SX_SAMPLE_REQUIRE(a->C >= 1 && a->C < (int64_t)1 << 31 && a->n >= 1 && a->n <= kWideFrom, "bad shape");
    SX_SAMPLE_REQUIRE(!resident || (a->fun_id >= 0 && a->fun_id < SX_FUN_COUNT), "unknown objective");
    SX_SAMPLE_REQUIRE(a->method == SX_SAMPLE_MCMC || a->method == SX_SAMPLE_HMC, "unknown method");
    SX_SAMPLE_REQUIRE(a->jac == SX_JAC_FINITE_DIFF || a->jac == SX_JAC_ANALYTIC, "unknown gradient mode");
    SX_SAMPLE_REQUIRE(a->rng == SX_RNG_PHILOX || (host_draws && a->rng == SX_RNG_HOST),
                      "unknown rng mode (around a caller's objective and on a ladder the draws are made in the kernels: "
                      "SX_RNG_PHILOX)");
    SX_SAMPLE_REQUIRE(a->maxiter >= 1 && a->maxiter < (int64_t)1 << 31 && it0 >= 0 && steps >= 0 && it0 + steps <= a->maxiter,
                      "samples outside [0, maxiter)");
    SX_SAMPLE_REQUIRE(a->rng != SX_RNG_HOST || (a->C == 1 && a->x0 && !a->reject && (a->maxiter == 1 || (a->normals && a->logu))),
                      "host draws serve one chain without feasibility rejection, and need x0, normals and logu");
    SX_SAMPLE_REQUIRE((a->xall == nullptr) == (a->funall == nullptr), "xall and funall go together");
    SX_SAMPLE_REQUIRE(a->x0 == nullptr || a->x0_stride == 0 || a->x0_stride >= a->n, "bad x0 stride");
    if (a->method == SX_SAMPLE_MCMC)
        SX_SAMPLE_REQUIRE(a->k >= 1 && a->k <= a->n, "block length outside [1, n]");
    else
        SX_SAMPLE_REQUIRE(a->nleap >= 1 && (!resident || a->jac == SX_JAC_ANALYTIC || a->fd_step != 0.0), "bad nleap / step");
    return 0;
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

// ---------------------------------------------------------------------------------------------------------------------
// The step of a chain.  The kernels differ in where a chain's rows live (LDS, device memory) and whether a padding row group
// may store: they pass that as functors (`put`, `step`) and keep their own loops over the rows.
// ---------------------------------------------------------------------------------------------------------------------
// element e of the chain's step: a.step[e] times the adapted multiplier s (the plain kernels do not multiply at all)
template <bool ADAPT>
__device__ __forceinline__ double chain_step(const sx_sample_args &a, double s, int e) {
    if constexpr (ADAPT)
        return s * a.step[e];
    else
        return a.step[e];
}

// Metropolis-Hastings, the proposal (mcmc/_mcmc.py:104-118): sample it >= 1 perturbs block (it - 1) mod nblocks of k
// consecutive variables, [j0, j1) (the last block is the shorter one when k does not divide n), by randn(j1 - j0) * step
__device__ __forceinline__ void mcmc_block(int64_t it, int n, int k, int nblocks, int &j0, int &j1) {
    j0 = (int)((it - 1) % nblocks) * k;
    j1 = j0 + k < n ? j0 + k : n;
}
// put(e, .) takes every element of the proposal: X[e] + z * step(e) inside the block, X[e] outside
template <int LPR, class Step, class Put>
__device__ __forceinline__ void mcmc_propose(const sx_sample_args &a, uint32_t chain, int64_t it, const double *X, int l,
                                             int j0, int j1, Step &&step, Put &&put) {
    const int n = a.n;
    for (int e0 = l; e0 < n; e0 += 2 * LPR) {  // element pairs (e0, e0 + LPR): one Box-Muller call
        const int e1 = e0 + LPR;
        const bool in0 = e0 >= j0 && e0 < j1, in1 = e1 >= j0 && e1 < j1;
        double z0 = 0.0, z1 = 0.0;
        if (in0 || in1) {  // (Philox draws: the reference's stream is read by the resident kernels alone)
            philox_normal_pair<LPR>(e0, chain, (uint32_t)it, kPurposeSampleProposal, a.key0, a.key1, z0, z1);
        }
        const double v0 = X[e0];
        put(e0, in0 ? v0 + z0 * step(e0) : v0);
        if (e1 < n) {
            const double v1 = X[e1];
            put(e1, in1 ? v1 + z1 * step(e1) : v1);
        }
    }
}

// The Metropolis decision on sample it >= 1 (mcmc/_mcmc.py:120-134, hmc/_hmc.py:159-172): a proposal of value fprop that
// passed the box test (`feasible`; any proposal without constraints) is accepted when min(0, d) > log(rand()), d its log
// acceptance ratio -- mcmc: fcur - fprop, on a tempered rung times beta; hmc: (fcur - fprop) + K0 - K.  Python's
// min(0.0, d): a NaN d gives 0.0 and accepts.  `mcmc` picks what the run returns as x, whose change xbest_changed reports:
// the best ACCEPTED sample (mcmc/_mcmc.py:155), or numpy's argmin over funall (hmc/_hmc.py:187).
struct Decision {
    bool accept = false, xbest_changed = false;
    double dstat = 0.0;  // d of a feasible proposal, 0.0 else: what adapt_update takes
};
__device__ __forceinline__ Decision chain_decide(ChainState &st, const sx_sample_args &a, uint32_t chain, int64_t it,
                                                 bool mcmc, bool feasible, double d, double fprop) {
    Decision r;
    if (feasible) {
        st.nfeas += 1;
        const double logu = philox_log_accept(chain, (uint32_t)it, a.key0, a.key1);
        r.accept = (d < 0.0 ? d : 0.0) > logu;
        r.dstat = d;
    }
    if (r.accept) {
        bool acc_best, arg_best;
        st.accept(fprop, it, acc_best, arg_best);
        r.xbest_changed = mcmc ? acc_best : arg_best;
    }
    return r;
}

// The tail of a sample AROUND a caller's objective (sx_sample_unfused.hip), the chain's rows in device memory: cur <- the
// proposal U when accepted; row `row` of xall / funall (when `record`) and xbest (when it changed) take the sample; the
// scalars go back to their arrays
template <int LPR>
__device__ __forceinline__ void commit_sample(const sx_sample_args &a, const ChainState &st, int64_t c, int l, const double *U,
                                              bool accept, bool xbest_changed, bool record, int64_t row) {
    const int n = a.n;
    double *X = a.cur + c * n;
    double *all = record ? a.xall + row * n : nullptr;
    for (int e = l; e < n; e += LPR) {
        const double v = accept ? U[e] : X[e];
        if (accept) X[e] = v;
        if (all != nullptr) st_stream(all + e, v);
        if (xbest_changed) a.xbest[c * n + e] = v;
    }
    if (l == 0) {
        if (all != nullptr) st_stream(a.funall + row, st.fcur);
        st.store(a, c);
    }
}

}  // namespace
}  // namespace sx
