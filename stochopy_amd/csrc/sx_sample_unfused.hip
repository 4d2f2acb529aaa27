// Samplers around a CALLER-SUPPLIED objective (factory.batched: the (P, n) device array in, (P,) values out).  The objective
// cannot be fused into the chain kernels of sx_sample.hip, so a sample is
//   mcmc: propose kernel -> caller's objective -> decide kernel
//   hmc:  propose kernel -> (nleap + 2) x (gradient -> leap kernel) -> caller's objective -> decide kernel
// where a gradient is the caller's own, or 2-point finite differences: fd_rows kernel -> caller's objective on the stacked
// rows -> fd_gradient kernel.  The mcmc proposal, the decision and the tail of a sample are sx_sample.hpp's functions, shared with
// the tempered ladders; they state the resident kernels' expressions (sx_sample.hip spells its own, for speed), under
// -ffp-contract=off: given bit-identical objective / gradient values the run is the resident run, bit for bit.  What is
// written HERE is where a chain's rows live (device memory, `if (active)` stores), the hmc momentum draw, the leap-frog step cut
// at the gradient, the finite-difference rows and the exchange of a ladder's states in memory.  State lives in sx_sample_args'
// per-chain arrays, which the resident kernels round-trip from launch to launch too.
//
// Parallel tempering (sx_sample_temper.hip) around such an objective: propose kernel -> caller's objective -> decide_tempered
// kernel -> on an exchange event the swap kernel (one row group per pair of neighbouring rungs, the states in device memory).
//
// One geometry for all these kernels: one row group of lanes_per_row(n) lanes per chain, lane l owns elements l, l + LPR, ...;
// padding row groups shadow the last chain for loads and store nothing; no LDS, no barrier, no atomics.  Philox draws only.
//
// Reference code replaced (paths relative to the reference checkout; the block's perturbation and the decisions are cited
// again at the function of sx_sample.hpp that states them):
//   stochopy/sample/mcmc/_mcmc.py:93, :106-118   initial point, the block's perturbation
//   stochopy/sample/mcmc/_mcmc.py:120-140        decision and bookkeeping after `fun(xnew)`
//   stochopy/sample/hmc/_hmc.py:124, :137-141    initial point, momentum and its kinetic energy
//   stochopy/sample/hmc/_hmc.py:143-155          leap-frog steps (sample_leap_kernel)
//   stochopy/sample/hmc/_hmc.py:157-172          decision and bookkeeping
//   stochopy/sample/hmc/_hmc.py:217-233          numerical_gradient (in-place perturb / restore: sample_fd_rows_kernel)
#include "sx_enqueue.hpp"
#include "sx_host.hpp"
#include "sx_rowops.hpp"
#include "sx_sample.hpp"

using namespace sx;

namespace {

// rows of one workgroup: the row kernels' 16-row cap, no LDS to fit
inline Geometry chain_geometry(int64_t C, int n) {
    const int waves = waves_per_workgroup(n, 0);
    const int rows = waves * (kWave / lanes_per_row(n));
    return Geometry{(unsigned)((C + rows - 1) / rows), (unsigned)(waves * kWave), 0};
}

// ADAPT, here and below: sx_sample_adapt as the kernel's last argument (sx_sample.hpp; without it an empty struct that is never
// read).  The propose and leap kernels need chain c's multiplier of a.step alone: ad.scale, 1.0 while nothing adapts.
// METRIC (sx_sample_metric, with ADAPT): element e of the chain's step is scale * eff, eff = m[c, e] * a.step[e] formed from
// the chain's row of m in device memory (metric_eff) -- the product the resident kernels keep in LDS.
template <bool ADAPT, bool METRIC>
__device__ __forceinline__ double chain_scale(const AdaptArg<ADAPT, METRIC> &ad, int64_t c) {
    if constexpr (ADAPT)
        if (ad.warmup > 0) return ad.scale[c];
    return 1.0;
}
template <bool ADAPT, bool METRIC>
__device__ __forceinline__ double unfused_step(const sx_sample_args &a, const AdaptArg<ADAPT, METRIC> &ad, double scale,
                                               int64_t c, int e) {
    if constexpr (METRIC)
        return scale * metric_eff(a, ad.mt, c, e);
    else
        return chain_step<ADAPT>(a, scale, e);
}

// sample `it`: the proposal (it = 0: the initial point) -> prop (C, n); hmc: momentum -> pmom (C, n), its kinetic energy -> k0 (C)
template <int LPR, bool ADAPT, bool METRIC>
__global__ __launch_bounds__(kMaxWavesPerBlock *kWave) void sample_propose_kernel(const sx_sample_args a, int64_t it,
                                                                                  double *__restrict__ prop,
                                                                                  double *__restrict__ pmom,
                                                                                  double *__restrict__ k0,
                                                                                  const AdaptArg<ADAPT, METRIC> ad) {
    const RowIds<LPR> id(a.C);
    const int n = a.n, l = id.l, k = a.k;
    const int64_t c = id.rowc;
    const bool active = id.active;
    // (sample 0 takes no step; its decide kernel writes the first multiplier)
    const double scale = it > 0 ? chain_scale<ADAPT, METRIC>(ad, c) : 1.0;
    const double *X = a.cur + c * n;
    double *U = prop + c * n;
    if (it == 0) {
        for (int e = l; e < n; e += LPR) {
            const double v = initial_value<LPR>(a, c, e);
            if (active) U[e] = v;
        }
    } else if (a.method == SX_SAMPLE_MCMC) {
        int j0, j1;
        mcmc_block(it, n, k, (n + k - 1) / k, j0, j1);
        mcmc_propose<LPR>(
            a, (uint32_t)c, it, X, l, j0, j1, [&](int e) { return unfused_step<ADAPT, METRIC>(a, ad, scale, c, e); },
            [&](int e, double v) {
                if (active) U[e] = v;
            });
    } else {
        double *Pm = pmom + c * n;
        double s = 0.0;  // (hmc_kernel's momentum draw, hmc/_hmc.py:137-141)
        for (int e0 = l; e0 < n; e0 += 2 * LPR) {
            const int e1 = e0 + LPR;
            double z0 = 0.0, z1 = 0.0;
            philox_normal_pair<LPR>(e0, (uint32_t)c, (uint32_t)it, kPurposeSampleMomentum, a.key0, a.key1, z0, z1);
            const double v0 = X[e0];
            if (active) U[e0] = v0, Pm[e0] = z0;
            s += z0 * z0;
            if (e1 < n) {
                const double v1 = X[e1];
                if (active) U[e1] = v1, Pm[e1] = z1;
                s += z1 * z1;
            }
        }
        const double K0 = 0.5 * row_sum<LPR>(s);
        if (active && l == 0) k0[c] = K0;
    }
}

// one momentum step with the gradient G, and the position step behind it when `move` (hmc/_hmc.py:143-155)
template <int LPR, bool ADAPT, bool METRIC>
__global__ __launch_bounds__(kMaxWavesPerBlock *kWave) void sample_leap_kernel(const sx_sample_args a, double coef, int move,
                                                                               double *__restrict__ q,
                                                                               double *__restrict__ pmom,
                                                                               const double *__restrict__ G,
                                                                               const AdaptArg<ADAPT, METRIC> ad) {
    const RowIds<LPR> id(a.C);
    const int n = a.n, l = id.l;
    const int64_t c = id.rowc;
    double *Q = q + c * n, *Pm = pmom + c * n;
    const double *g = G + c * n;
    const double scale = chain_scale<ADAPT, METRIC>(ad, c);
    for (int e = l; e < n; e += LPR) {
        const double gv = g[e];
        const double st = unfused_step<ADAPT, METRIC>(a, ad, scale, c, e);
        const double p = Pm[e] - (coef * st) * gv;
        const double qn = Q[e] + st * p;
        if (id.active) {
            Pm[e] = p;
            if (move) Q[e] = qn;
        }
    }
}

// The rows numerical_gradient evaluates for axes [axis0, axis0 + naxes): the reference moves component i of its two copies by
// +-h and moves it BACK in place, so at axis i the components before i carry that round trip.  W (naxes, 2, C, n): [.,0] the
// +h copy (x2), [.,1] the -h copy (x1).  blockIdx.y is the axis within the chunk.
template <int LPR>
__global__ __launch_bounds__(kMaxWavesPerBlock *kWave) void sample_fd_rows_kernel(const sx_sample_args a,
                                                                                  const double *__restrict__ q, int axis0,
                                                                                  double *__restrict__ W) {
    const RowIds<LPR> id(a.C);
    if (!id.active) return;
    const int n = a.n, l = id.l;
    const int64_t c = id.row, ia = blockIdx.y;
    const int i = axis0 + (int)ia;
    const double h = a.fd_step;
    const double *Q = q + c * n;
    double *X2 = W + ((ia * 2 + 0) * a.C + c) * n, *X1 = W + ((ia * 2 + 1) * a.C + c) * n;
    for (int e = l; e < n; e += LPR) {
        const double v = Q[e];
        double x1 = v - h, x2 = v + h;
        if (e < i) {
            x1 = x1 + h;
            x2 = x2 - h;
        }
        st_stream(X2 + e, e <= i ? x2 : v);
        st_stream(X1 + e, e <= i ? x1 : v);
    }
}

// fW (naxes, 2, C) the values of those rows -> G[c, axis0 + ia]
template <int LPR>
__global__ __launch_bounds__(kMaxWavesPerBlock *kWave) void sample_fd_gradient_kernel(const sx_sample_args a,
                                                                                      const double *__restrict__ fW, int axis0,
                                                                                      int naxes, double *__restrict__ G) {
    const RowIds<LPR> id(a.C);
    if (!id.active) return;
    const int64_t c = id.row;
    const double h = a.fd_step;
    for (int ia = id.l; ia < naxes; ia += LPR) {
        const double f2 = fW[((int64_t)ia * 2 + 0) * a.C + c], f1 = fW[((int64_t)ia * 2 + 1) * a.C + c];
        G[c * a.n + axis0 + ia] = (0.5 * (f2 - f1)) / h;
    }
}

// the decision on sample `it` with the proposal's value fprop (C), and the chain's bookkeeping
template <int LPR, bool ADAPT, bool METRIC>
__global__ __launch_bounds__(kMaxWavesPerBlock *kWave) void sample_decide_kernel(const sx_sample_args a, int64_t it,
                                                                                 const double *__restrict__ prop,
                                                                                 const double *__restrict__ fprop,
                                                                                 const double *__restrict__ pmom,
                                                                                 const double *__restrict__ k0,
                                                                                 const AdaptArg<ADAPT, METRIC> ad) {
    const RowIds<LPR> id(a.C);
    const int n = a.n, l = id.l;
    const int64_t c = id.rowc;
    const double *U = prop + c * n;
    const bool mcmc = a.method == SX_SAMPLE_MCMC;
    const double fU = fprop[c];
    ChainState st;
    AdaptState as;
    Decision r{true, true, 0.0};  // (sample 0: cur = the initial point)
    if (it == 0) {
        st.start(fU);
        if constexpr (ADAPT) as.start();
        if constexpr (METRIC) {
            double sbase;
            metric_start<LPR>(a, ad.mt, c, l, id.active, sbase);
        }
    } else {
        st.load(a, c);
        if constexpr (ADAPT) as.load(ad, c);
        double K0 = 0.0, K = 0.0;
        if (!mcmc) {
            K0 = k0[c];
            const double *Pm = pmom + c * n;
            double s = 0.0;
            for (int e = l; e < n; e += LPR) s += Pm[e] * Pm[e];
            K = 0.5 * row_sum<LPR>(s);
        }
        const bool feasible = !a.reject || row_in_box<LPR>(a, U, n, l);
        r = chain_decide(st, a, (uint32_t)c, it, mcmc, feasible, mcmc ? st.fcur - fU : ((st.fcur - fU) + K0) - K, fU);
        if constexpr (METRIC) {  // (the chain's state after this decision: cur is committed below; eff is formed from m)
            const double *X = a.cur + c * n;
            const bool accepted = r.accept;
            double sbase = metric_load_sbase(ad.mt, c);
            metric_update<LPR>(
                a, ad, as, sbase, c, l, id.active, it, feasible, r.dstat, st.nacc,
                [&](int e) { return accepted ? U[e] : X[e]; }, [](int, double) {});
        } else if constexpr (ADAPT) {
            adapt_update(as, ad.warmup, ad.target, it, feasible, r.dstat, st.nacc);
        }
    }
    if (!id.active) return;
    bool record = a.xall != nullptr;
    int64_t row = c * a.maxiter + it;
    if constexpr (ADAPT) {
        int64_t rec = 0;
        record = record && adapt_record(ad, it, rec);
        row = c * ad.rec_rows + rec;
    }
    commit_sample<LPR>(a, st, c, l, U, r.accept, r.xbest_changed, record, row);
    if constexpr (ADAPT)
        if (l == 0) as.store(ad, c);
}

// Parallel tempering (sx_sample_temper.hip) around a caller's objective: the decision of replica c = ladder * K + rung with
// d = (fcur - fprop) * beta[rung].  record = 0: row `it` of xall / funall is left to sample_swap_kernel (an exchange of
// rungs (0, 1) follows); else the cold rungs write it at their LADDER's index.  mcmc only.
template <int LPR>
__global__ __launch_bounds__(kMaxWavesPerBlock *kWave) void sample_decide_tempered_kernel(const sx_sample_args a, int64_t it,
                                                                                          const double *__restrict__ prop,
                                                                                          const double *__restrict__ fprop,
                                                                                          const double *__restrict__ beta, int K,
                                                                                          int record) {
    const RowIds<LPR> id(a.C);
    const int n = a.n, l = id.l;
    const int64_t c = id.rowc;
    const int rung = (int)(c % K);
    const double *U = prop + c * n;
    const double fU = fprop[c];
    ChainState st;
    Decision r{true, true, 0.0};  // (sample 0: cur = the initial point)
    if (it == 0) {
        st.start(fU);
    } else {
        st.load(a, c);
        const bool feasible = !a.reject || row_in_box<LPR>(a, U, n, l);
        r = chain_decide(st, a, (uint32_t)c, it, true, feasible, (st.fcur - fU) * beta[rung], fU);
    }
    if (!id.active) return;
    commit_sample<LPR>(a, st, c, l, U, r.accept, r.xbest_changed, a.xall != nullptr && record && rung == 0,
                       (c / K) * a.maxiter + it);
}

// Exchange event j after sample `it`: one row group per PAIR (pairs = ladders * pairs_per_ladder; the lower rungs are
// first, first + 2, ...), the states in device memory.  The pair of rungs (0, 1) writes row `it` of xall / funall.
template <int LPR>
__global__ __launch_bounds__(kMaxWavesPerBlock *kWave) void sample_swap_kernel(const sx_sample_args a, int64_t it,
                                                                               const double *__restrict__ beta, int K,
                                                                               int first, int pairs_per_ladder, int64_t pairs,
                                                                               int64_t *__restrict__ nswap) {
    const RowIds<LPR> id(pairs);
    if (!id.active) return;
    const int n = a.n, l = id.l;
    const int64_t ladder = id.row / pairs_per_ladder;
    const int kl = first + 2 * (int)(id.row - ladder * pairs_per_ladder);
    const int64_t ql = ladder * K + kl, qu = ql + 1;
    const double fl = a.fcur[ql], fu = a.fcur[qu];
    const bool swap = tempered_swap(fl, fu, beta[kl], beta[kl + 1], (uint32_t)ql, (uint32_t)it, a.key0, a.key1);
    double *Xl = a.cur + ql * n, *Xu = a.cur + qu * n;
    bool best_l = false, best_u = false;
    if (swap) {
        ChainState sl, su;
        sl.load(a, ql);
        su.load(a, qu);
        sl.arrive(fu, it, best_l);
        su.arrive(fl, it, best_u);
        if (l == 0) {
            sl.store(a, ql);
            su.store(a, qu);
            nswap[ql] += 1;
        }
    }
    double *all = (a.xall != nullptr && kl == 0) ? a.xall + (ladder * a.maxiter + it) * n : nullptr;
    for (int e = l; e < n; e += LPR) {
        const double vl = Xl[e], vu = Xu[e];
        if (swap) {
            Xl[e] = vu;
            Xu[e] = vl;
            if (best_l) a.xbest[ql * n + e] = vu;
            if (best_u) a.xbest[qu * n + e] = vl;
        }
        if (all != nullptr) st_stream(all + e, swap ? vu : vl);
    }
    if (all != nullptr && l == 0) st_stream(a.funall + ladder * a.maxiter + it, swap ? fu : fl);
}

// What every entry point `who` does first, for its sample `it` (the entry points without one pass 0): sx_sample_run's
// conditions on the arguments these kernels read, and those on `ad` for the adapting / thinning forms
template <bool ADAPT = false, bool METRIC = false>
int check_entry(const char *who, const sx_sample_args *a, int64_t it, const sx_sample_adapt *ad = nullptr,
                const sx_sample_metric *mt = nullptr) {
    return (check_sample_args(who, a, it, 1, false, false) || (ADAPT && check_adapt(a, ad)) || (METRIC && check_metric(ad, mt)))
               ? -1
               : 0;
}

// each plain entry point, its *_adapt and its *_metric form: one body
template <bool ADAPT, bool METRIC = false>
int propose(const char *who, const sx_sample_args *a, const sx_sample_adapt *ad, const sx_sample_metric *mt, int64_t it, double *prop, double *pmom,
            double *k0, void *stream) {
    if (check_entry<ADAPT, METRIC>(who, a, it, ad, mt)) return -1;
    SX_SAMPLE_REQUIRE(prop != nullptr, "null proposal array");
    SX_SAMPLE_REQUIRE(a->method == SX_SAMPLE_MCMC || it == 0 || (pmom && k0), "hmc needs pmom and k0");
    const Geometry g = chain_geometry(a->C, a->n);
    Enqueue q((hipStream_t)stream);
    SX_DISPATCH_LPR(a->n, return q.kernel(sample_propose_kernel<LPR, ADAPT, METRIC>, dim3(g.blocks), dim3(g.threads), 0, *a, it, prop,
                                          pmom, k0, adapt_arg<ADAPT, METRIC>(ad, mt)))
    return -1;
}

template <bool ADAPT, bool METRIC = false>
int leap(const char *who, const sx_sample_args *a, const sx_sample_adapt *ad, const sx_sample_metric *mt, double coef, int move, double *q, double *pmom,
         const double *G, void *stream) {
    if (check_entry<ADAPT, METRIC>(who, a, 0, ad, mt)) return -1;
    SX_SAMPLE_REQUIRE(a->method == SX_SAMPLE_HMC && q && pmom && G, "hmc with q, pmom and G");
    const Geometry g = chain_geometry(a->C, a->n);
    Enqueue sink((hipStream_t)stream);
    SX_DISPATCH_LPR(a->n, return sink.kernel(sample_leap_kernel<LPR, ADAPT, METRIC>, dim3(g.blocks), dim3(g.threads), 0, *a, coef, move, q,
                                             pmom, G, adapt_arg<ADAPT, METRIC>(ad, mt)))
    return -1;
}

template <bool ADAPT, bool METRIC = false>
int decide(const char *who, const sx_sample_args *a, const sx_sample_adapt *ad, const sx_sample_metric *mt, int64_t it, const double *prop,
           const double *fprop, const double *pmom, const double *k0, void *stream) {
    if (check_entry<ADAPT, METRIC>(who, a, it, ad, mt)) return -1;
    SX_SAMPLE_REQUIRE(prop && fprop, "null proposal / value array");
    SX_SAMPLE_REQUIRE(a->method == SX_SAMPLE_MCMC || it == 0 || (pmom && k0), "hmc needs pmom and k0");
    const Geometry g = chain_geometry(a->C, a->n);
    Enqueue q((hipStream_t)stream);
    SX_DISPATCH_LPR(a->n, return q.kernel(sample_decide_kernel<LPR, ADAPT, METRIC>, dim3(g.blocks), dim3(g.threads), 0, *a, it, prop,
                                          fprop, pmom, k0, adapt_arg<ADAPT, METRIC>(ad, mt)))
    return -1;
}

}  // namespace

extern "C" int sx_sample_propose(const sx_sample_args *a, int64_t it, double *prop, double *pmom, double *k0, void *stream) {
    return propose<false>("sx_sample_propose", a, nullptr, nullptr, it, prop, pmom, k0, stream);
}
extern "C" int sx_sample_leap(const sx_sample_args *a, double coef, int move, double *q, double *pmom, const double *G,
                              void *stream) {
    return leap<false>("sx_sample_leap", a, nullptr, nullptr, coef, move, q, pmom, G, stream);
}
extern "C" int sx_sample_decide(const sx_sample_args *a, int64_t it, const double *prop, const double *fprop,
                                const double *pmom, const double *k0, void *stream) {
    return decide<false>("sx_sample_decide", a, nullptr, nullptr, it, prop, fprop, pmom, k0, stream);
}

// The adapting / thinning forms (sx_sample_adapt)
extern "C" int sx_sample_propose_adapt(const sx_sample_args *a, const sx_sample_adapt *ad, int64_t it, double *prop,
                                       double *pmom, double *k0, void *stream) {
    return propose<true>("sx_sample_propose_adapt", a, ad, nullptr, it, prop, pmom, k0, stream);
}
extern "C" int sx_sample_leap_adapt(const sx_sample_args *a, const sx_sample_adapt *ad, double coef, int move, double *q,
                                    double *pmom, const double *G, void *stream) {
    return leap<true>("sx_sample_leap_adapt", a, ad, nullptr, coef, move, q, pmom, G, stream);
}
extern "C" int sx_sample_decide_adapt(const sx_sample_args *a, const sx_sample_adapt *ad, int64_t it, const double *prop,
                                      const double *fprop, const double *pmom, const double *k0, void *stream) {
    return decide<true>("sx_sample_decide_adapt", a, ad, nullptr, it, prop, fprop, pmom, k0, stream);
}

// The forms with per-axis scales (sx_sample_metric)
extern "C" int sx_sample_propose_metric(const sx_sample_args *a, const sx_sample_adapt *ad, const sx_sample_metric *mt, int64_t it,
                                        double *prop, double *pmom, double *k0, void *stream) {
    return propose<true, true>("sx_sample_propose_metric", a, ad, mt, it, prop, pmom, k0, stream);
}
extern "C" int sx_sample_leap_metric(const sx_sample_args *a, const sx_sample_adapt *ad, const sx_sample_metric *mt, double coef,
                                     int move, double *q, double *pmom, const double *G, void *stream) {
    return leap<true, true>("sx_sample_leap_metric", a, ad, mt, coef, move, q, pmom, G, stream);
}
extern "C" int sx_sample_decide_metric(const sx_sample_args *a, const sx_sample_adapt *ad, const sx_sample_metric *mt, int64_t it,
                                       const double *prop, const double *fprop, const double *pmom, const double *k0,
                                       void *stream) {
    return decide<true, true>("sx_sample_decide_metric", a, ad, mt, it, prop, fprop, pmom, k0, stream);
}

extern "C" int sx_sample_fd_rows(const sx_sample_args *a, const double *q, int axis0, int naxes, double *W, void *stream) {
    const char *who = "sx_sample_fd_rows";
    if (check_entry(who, a, 0)) return -1;
    SX_SAMPLE_REQUIRE(a->method == SX_SAMPLE_HMC && q && W && a->fd_step != 0.0, "hmc with q, W and a step");
    SX_SAMPLE_REQUIRE(axis0 >= 0 && naxes >= 1 && axis0 <= a->n - naxes, "axes outside [0, n)");
    const Geometry g = chain_geometry(a->C, a->n);
    Enqueue sink((hipStream_t)stream);
    SX_DISPATCH_LPR(a->n, return sink.kernel(sample_fd_rows_kernel<LPR>, dim3(g.blocks, (unsigned)naxes), dim3(g.threads), 0, *a, q,
                                             axis0, W))
    return -1;
}

extern "C" int sx_sample_fd_gradient(const sx_sample_args *a, const double *fW, int axis0, int naxes, double *G,
                                     void *stream) {
    const char *who = "sx_sample_fd_gradient";
    if (check_entry(who, a, 0)) return -1;
    SX_SAMPLE_REQUIRE(a->method == SX_SAMPLE_HMC && fW && G && a->fd_step != 0.0, "hmc with fW, G and a step");
    SX_SAMPLE_REQUIRE(axis0 >= 0 && naxes >= 1 && axis0 <= a->n - naxes, "axes outside [0, n)");
    const Geometry g = chain_geometry(a->C, a->n);
    Enqueue q((hipStream_t)stream);
    SX_DISPATCH_LPR(a->n, return q.kernel(sample_fd_gradient_kernel<LPR>, dim3(g.blocks), dim3(g.threads), 0, *a, fW, axis0, naxes, G))
    return -1;
}

extern "C" int sx_sample_decide_tempered(const sx_sample_args *a, int64_t it, const double *prop, const double *fprop,
                                         const double *beta, int K, int record, void *stream) {
    const char *who = "sx_sample_decide_tempered";
    if (check_entry(who, a, it)) return -1;
    SX_SAMPLE_REQUIRE(prop && fprop && beta, "null proposal / value / beta array");
    SX_SAMPLE_REQUIRE(a->method == SX_SAMPLE_MCMC, "mcmc only");
    SX_SAMPLE_REQUIRE(K >= 2 && a->C % K == 0, "C is ladders x K replicas, K >= 2");
    const Geometry g = chain_geometry(a->C, a->n);
    Enqueue q((hipStream_t)stream);
    SX_DISPATCH_LPR(a->n, return q.kernel(sample_decide_tempered_kernel<LPR>, dim3(g.blocks), dim3(g.threads), 0, *a, it, prop,
                                          fprop, beta, K, record))
    return -1;
}

extern "C" int sx_sample_swap(const sx_sample_args *a, int64_t it, int64_t j, const double *beta, int K, int64_t *nswap,
                              void *stream) {
    const char *who = "sx_sample_swap";
    if (check_entry(who, a, it)) return -1;
    SX_SAMPLE_REQUIRE(beta && nswap, "null beta / nswap array");
    SX_SAMPLE_REQUIRE(a->method == SX_SAMPLE_MCMC, "mcmc only");
    SX_SAMPLE_REQUIRE(K >= 2 && a->C % K == 0 && it >= 1 && j >= 1, "C is ladders x K replicas, K >= 2; it, j >= 1");
    const int first = (int)((j + 1) & 1);
    const int pairs_per_ladder = (K - first) / 2;
    if (pairs_per_ladder == 0) return 0;  // (K = 2 at an even event: nobody has a partner)
    const int64_t pairs = (a->C / K) * pairs_per_ladder;
    const Geometry g = chain_geometry(pairs, a->n);
    Enqueue q((hipStream_t)stream);
    SX_DISPATCH_LPR(a->n, return q.kernel(sample_swap_kernel<LPR>, dim3(g.blocks), dim3(g.threads), 0, *a, it, beta, K, first,
                                          pairs_per_ladder, pairs, nswap))
    return -1;
}
