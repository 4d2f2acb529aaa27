// Samplers around a CALLER-SUPPLIED objective (factory.batched: the (P, n) device array in, (P,) values out).  The objective
// cannot be fused into the chain kernels of sx_sample.hip, so a sample is
//   mcmc: propose kernel -> caller's objective -> decide kernel
//   hmc:  propose kernel -> (nleap + 2) x (gradient -> leap kernel) -> caller's objective -> decide kernel
// where a gradient is the caller's own, or 2-point finite differences: fd_rows kernel -> caller's objective on the stacked
// rows -> fd_gradient kernel.  Draws, arithmetic and bookkeeping are the resident kernels' (sx_sample.hpp, the same
// expressions under -ffp-contract=off): given bit-identical objective / gradient values the run is the resident run, bit for
// bit.  State lives in sx_sample_args' per-chain arrays, which the resident kernels round-trip from launch to launch too.
//
// Parallel tempering (sx_sample_temper.hip) around such an objective: propose kernel -> caller's objective -> decide_tempered
// kernel -> on an exchange event the swap kernel (one row group per pair of neighbouring rungs, the states in device memory).
//
// One geometry for all these kernels: one row group of lanes_per_row(n) lanes per chain, lane l owns elements l, l + LPR, ...;
// padding row groups shadow the last chain for loads and store nothing; no LDS, no barrier, no atomics.  Philox draws only.
//
// Reference code replaced (paths relative to the reference checkout):
//   stochopy/sample/mcmc/_mcmc.py:93, :106-118   initial point, the block's perturbation
//   stochopy/sample/mcmc/_mcmc.py:120-140        decision and bookkeeping after `fun(xnew)`
//   stochopy/sample/hmc/_hmc.py:124, :137-141    initial point, momentum and its kinetic energy
//   stochopy/sample/hmc/_hmc.py:143-155          leap-frog steps
//   stochopy/sample/hmc/_hmc.py:157-172          decision and bookkeeping
//   stochopy/sample/hmc/_hmc.py:217-233          numerical_gradient (in-place perturb / restore)
#include "sx_enqueue.hpp"
#include "sx_host.hpp"
#include "sx_rowops.hpp"
#include "sx_sample.hpp"

using namespace sx;

namespace {

// rows of one workgroup: the row kernels' 16-row cap, no LDS to fit
inline Geometry chain_geometry(int64_t C, int n) {
    const int rpw = kWave / lanes_per_row(n);
    int waves = 1;
    while (2 * waves <= kMaxWavesPerBlock && 2 * waves * rpw <= kMaxRowsPerBlock) waves *= 2;
    const int rows = waves * rpw;
    return Geometry{(unsigned)((C + rows - 1) / rows), (unsigned)(waves * kWave), 0};
}

// sample `it`: the proposal (it = 0: the initial point) -> prop (C, n); hmc: momentum -> pmom (C, n), its kinetic energy -> k0 (C)
// (ADAPT, here and below: sx_sample_adapt -- the chain's multiplier of a.step, read from ad.scale; see sx_sample.hpp)
template <int LPR, bool ADAPT>
__device__ __forceinline__ void sample_propose(const sx_sample_args &a, const sx_sample_adapt &ad, int64_t it,
                                               double *__restrict__ prop, double *__restrict__ pmom,
                                               double *__restrict__ k0) {
    const RowIds<LPR> id(a.C);
    const int n = a.n, l = id.l, k = a.k;
    const int64_t c = id.rowc;
    double scale = 1.0;
    if constexpr (ADAPT)
        if (it > 0 && ad.warmup > 0) scale = ad.scale[c];
    const auto step = [&](int e) {
        if constexpr (ADAPT)
            return scale * a.step[e];
        else
            return a.step[e];
    };
    const double *X = a.cur + c * n;
    double *U = prop + c * n;
    if (it == 0) {
        for (int e = l; e < n; e += LPR) {
            const double v = initial_value<LPR>(a, c, e);
            if (id.active) U[e] = v;
        }
    } else if (a.method == SX_SAMPLE_MCMC) {
        const int nblocks = (n + k - 1) / k;
        const int j0 = (int)((it - 1) % nblocks) * k;
        const int j1 = j0 + k < n ? j0 + k : n;
        for (int e0 = l; e0 < n; e0 += 2 * LPR) {  // element pairs (e0, e0 + LPR): one Box-Muller call
            const int e1 = e0 + LPR;
            const bool in0 = e0 >= j0 && e0 < j1, in1 = e1 >= j0 && e1 < j1;
            double z0 = 0.0, z1 = 0.0;
            if (in0 || in1)
                philox_normal_pair<LPR>(e0, (uint32_t)c, (uint32_t)it, kPurposeSampleProposal, a.key0, a.key1, z0, z1);
            const double v0 = X[e0];
            const double u0 = in0 ? v0 + z0 * step(e0) : v0;
            if (id.active) U[e0] = u0;
            if (e1 < n) {
                const double v1 = X[e1];
                const double u1 = in1 ? v1 + z1 * step(e1) : v1;
                if (id.active) U[e1] = u1;
            }
        }
    } else {
        double *Pm = pmom + c * n;
        double s = 0.0;
        for (int e0 = l; e0 < n; e0 += 2 * LPR) {
            const int e1 = e0 + LPR;
            double z0 = 0.0, z1 = 0.0;
            philox_normal_pair<LPR>(e0, (uint32_t)c, (uint32_t)it, kPurposeSampleMomentum, a.key0, a.key1, z0, z1);
            const double v0 = X[e0];
            if (id.active) U[e0] = v0, Pm[e0] = z0;
            s += z0 * z0;
            if (e1 < n) {
                const double v1 = X[e1];
                if (id.active) U[e1] = v1, Pm[e1] = z1;
                s += z1 * z1;
            }
        }
        const double K0 = 0.5 * row_sum<LPR>(s);
        if (id.active && l == 0) k0[c] = K0;
    }
}
template <int LPR>
__global__ __launch_bounds__(kMaxWavesPerBlock *kWave) void sample_propose_kernel(const sx_sample_args a, int64_t it,
                                                                                  double *__restrict__ prop,
                                                                                  double *__restrict__ pmom,
                                                                                  double *__restrict__ k0) {
    sample_propose<LPR, false>(a, sx_sample_adapt{}, it, prop, pmom, k0);
}
template <int LPR>
__global__ __launch_bounds__(kMaxWavesPerBlock *kWave) void sample_propose_adapt_kernel(const sx_sample_args a,
                                                                                        const sx_sample_adapt ad, int64_t it,
                                                                                        double *__restrict__ prop,
                                                                                        double *__restrict__ pmom,
                                                                                        double *__restrict__ k0) {
    sample_propose<LPR, true>(a, ad, it, prop, pmom, k0);
}

// one momentum step with the gradient G, and the position step behind it when `move`
template <int LPR, bool ADAPT>
__device__ __forceinline__ void sample_leap(const sx_sample_args &a, const sx_sample_adapt &ad, double coef, int move,
                                            double *__restrict__ q, double *__restrict__ pmom, const double *__restrict__ G) {
    const RowIds<LPR> id(a.C);
    const int n = a.n, l = id.l;
    const int64_t c = id.rowc;
    double *Q = q + c * n, *Pm = pmom + c * n;
    const double *g = G + c * n;
    double scale = 1.0;
    if constexpr (ADAPT)
        if (ad.warmup > 0) scale = ad.scale[c];
    for (int e = l; e < n; e += LPR) {
        const double gv = g[e];
        double st = a.step[e];
        if constexpr (ADAPT) st = scale * st;
        const double p = Pm[e] - (coef * st) * gv;
        const double qn = Q[e] + st * p;
        if (id.active) {
            Pm[e] = p;
            if (move) Q[e] = qn;
        }
    }
}
template <int LPR>
__global__ __launch_bounds__(kMaxWavesPerBlock *kWave) void sample_leap_kernel(const sx_sample_args a, double coef, int move,
                                                                               double *__restrict__ q,
                                                                               double *__restrict__ pmom,
                                                                               const double *__restrict__ G) {
    sample_leap<LPR, false>(a, sx_sample_adapt{}, coef, move, q, pmom, G);
}
template <int LPR>
__global__ __launch_bounds__(kMaxWavesPerBlock *kWave) void sample_leap_adapt_kernel(const sx_sample_args a,
                                                                                     const sx_sample_adapt ad, double coef,
                                                                                     int move, double *__restrict__ q,
                                                                                     double *__restrict__ pmom,
                                                                                     const double *__restrict__ G) {
    sample_leap<LPR, true>(a, ad, coef, move, q, pmom, G);
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
template <int LPR, bool ADAPT>
__device__ __forceinline__ void sample_decide(const sx_sample_args &a, const sx_sample_adapt &ad, int64_t it,
                                              const double *__restrict__ prop, const double *__restrict__ fprop,
                                              const double *__restrict__ pmom, const double *__restrict__ k0) {
    const RowIds<LPR> id(a.C);
    const int n = a.n, l = id.l;
    const int64_t c = id.rowc;
    const double *U = prop + c * n;
    double *X = a.cur + c * n;
    const bool mcmc = a.method == SX_SAMPLE_MCMC;
    const double fU = fprop[c];
    ChainState st;
    AdaptState as;
    bool accept = false, xbest_changed = false;
    if (it == 0) {
        st.start(fU);
        if constexpr (ADAPT) as.start();
        accept = true;  // (cur = the initial point)
        xbest_changed = true;
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
        double dstat = 0.0;
        if (feasible) {
            st.nfeas += 1;
            const double logu = philox_log_accept((uint32_t)c, (uint32_t)it, a.key0, a.key1);
            const double d = mcmc ? st.fcur - fU : ((st.fcur - fU) + K0) - K;
            accept = (d < 0.0 ? d : 0.0) > logu;  // Python's min(0.0, d): a NaN d gives 0.0
            dstat = d;
        }
        if (accept) {
            bool acc_best, arg_best;
            st.accept(fU, it, acc_best, arg_best);
            xbest_changed = mcmc ? acc_best : arg_best;
        }
        if constexpr (ADAPT) adapt_update(as, ad.warmup, ad.target, it, feasible, dstat, st.nacc);
    }
    if (!id.active) return;
    bool record = a.xall != nullptr;
    int64_t row = c * a.maxiter + it;
    if constexpr (ADAPT) {
        int64_t r = 0;
        record = record && adapt_record(ad, it, r);
        row = c * ad.rec_rows + r;
    }
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
        if constexpr (ADAPT) as.store(ad, c);
    }
}
template <int LPR>
__global__ __launch_bounds__(kMaxWavesPerBlock *kWave) void sample_decide_kernel(const sx_sample_args a, int64_t it,
                                                                                 const double *__restrict__ prop,
                                                                                 const double *__restrict__ fprop,
                                                                                 const double *__restrict__ pmom,
                                                                                 const double *__restrict__ k0) {
    sample_decide<LPR, false>(a, sx_sample_adapt{}, it, prop, fprop, pmom, k0);
}
template <int LPR>
__global__ __launch_bounds__(kMaxWavesPerBlock *kWave) void sample_decide_adapt_kernel(const sx_sample_args a,
                                                                                       const sx_sample_adapt ad, int64_t it,
                                                                                       const double *__restrict__ prop,
                                                                                       const double *__restrict__ fprop,
                                                                                       const double *__restrict__ pmom,
                                                                                       const double *__restrict__ k0) {
    sample_decide<LPR, true>(a, ad, it, prop, fprop, pmom, k0);
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
    double *X = a.cur + c * n;
    const double fU = fprop[c];
    ChainState st;
    bool accept = false, xbest_changed = false;
    if (it == 0) {
        st.start(fU);
        accept = true;  // (cur = the initial point)
        xbest_changed = true;
    } else {
        st.load(a, c);
        const bool feasible = !a.reject || row_in_box<LPR>(a, U, n, l);
        if (feasible) {
            st.nfeas += 1;
            const double logu = philox_log_accept((uint32_t)c, (uint32_t)it, a.key0, a.key1);
            const double d = (st.fcur - fU) * beta[rung];
            accept = (d < 0.0 ? d : 0.0) > logu;
        }
        if (accept) {
            bool arg_best;
            st.accept(fU, it, xbest_changed, arg_best);
        }
    }
    if (!id.active) return;
    const int64_t ladder = c / K;
    double *all = (a.xall != nullptr && record && rung == 0) ? a.xall + (ladder * a.maxiter + it) * n : nullptr;
    for (int e = l; e < n; e += LPR) {
        const double v = accept ? U[e] : X[e];
        if (accept) X[e] = v;
        if (all != nullptr) st_stream(all + e, v);
        if (xbest_changed) a.xbest[c * n + e] = v;
    }
    if (l == 0) {
        if (all != nullptr) st_stream(a.funall + ladder * a.maxiter + it, st.fcur);
        st.store(a, c);
    }
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

// sx_sample_run's conditions on the arguments these kernels read
int check_args(const sx_sample_args *a, int64_t it) {
    SX_REQUIRE(a != nullptr, "sx_sample (unfused): null args");
    SX_REQUIRE(a->cur && a->fcur && a->facc && a->fmin && a->xbest && a->iacc && a->imin && a->nacc && a->nfeas,
               "sx_sample (unfused): null state pointer");
    SX_REQUIRE(a->lower && a->upper && a->step, "sx_sample (unfused): bounds / step missing");
    SX_REQUIRE(a->C >= 1 && a->C < (int64_t)1 << 31 && a->n >= 1 && a->n <= kWideFrom, "sx_sample (unfused): bad shape");
    SX_REQUIRE(a->method == SX_SAMPLE_MCMC || a->method == SX_SAMPLE_HMC, "sx_sample (unfused): unknown method");
    SX_REQUIRE(a->jac == SX_JAC_FINITE_DIFF || a->jac == SX_JAC_ANALYTIC, "sx_sample (unfused): unknown gradient mode");
    SX_REQUIRE(a->rng == SX_RNG_PHILOX, "sx_sample (unfused): the draws are made in the kernels (SX_RNG_PHILOX)");
    SX_REQUIRE(a->maxiter >= 1 && a->maxiter < (int64_t)1 << 31 && it >= 0 && it < a->maxiter,
               "sx_sample (unfused): sample outside [0, maxiter)");
    SX_REQUIRE((a->xall == nullptr) == (a->funall == nullptr), "sx_sample (unfused): xall and funall go together");
    SX_REQUIRE(a->x0 == nullptr || a->x0_stride == 0 || a->x0_stride >= a->n, "sx_sample (unfused): bad x0 stride");
    if (a->method == SX_SAMPLE_MCMC)
        SX_REQUIRE(a->k >= 1 && a->k <= a->n, "sx_sample (unfused): block length outside [1, n]");
    else
        SX_REQUIRE(a->nleap >= 1, "sx_sample (unfused): bad nleap");
    return 0;
}

}  // namespace

extern "C" int sx_sample_propose(const sx_sample_args *a, int64_t it, double *prop, double *pmom, double *k0, void *stream) {
    if (check_args(a, it)) return -1;
    SX_REQUIRE(prop != nullptr, "sx_sample_propose: null proposal array");
    SX_REQUIRE(a->method == SX_SAMPLE_MCMC || it == 0 || (pmom && k0), "sx_sample_propose: hmc needs pmom and k0");
    const Geometry g = chain_geometry(a->C, a->n);
    SX_DISPATCH_LPR(a->n, hipLaunchKernelGGL((sample_propose_kernel<LPR>), dim3(g.blocks), dim3(g.threads), 0,
                                             (hipStream_t)stream, *a, it, prop, pmom, k0))
    SX_LAUNCH_CHECK();
    return 0;
}

extern "C" int sx_sample_leap(const sx_sample_args *a, double coef, int move, double *q, double *pmom, const double *G,
                              void *stream) {
    if (check_args(a, 0)) return -1;
    SX_REQUIRE(a->method == SX_SAMPLE_HMC && q && pmom && G, "sx_sample_leap: hmc with q, pmom and G");
    const Geometry g = chain_geometry(a->C, a->n);
    SX_DISPATCH_LPR(a->n, hipLaunchKernelGGL((sample_leap_kernel<LPR>), dim3(g.blocks), dim3(g.threads), 0,
                                             (hipStream_t)stream, *a, coef, move, q, pmom, G))
    SX_LAUNCH_CHECK();
    return 0;
}

extern "C" int sx_sample_fd_rows(const sx_sample_args *a, const double *q, int axis0, int naxes, double *W, void *stream) {
    if (check_args(a, 0)) return -1;
    SX_REQUIRE(a->method == SX_SAMPLE_HMC && q && W && a->fd_step != 0.0, "sx_sample_fd_rows: hmc with q, W and a step");
    SX_REQUIRE(axis0 >= 0 && naxes >= 1 && axis0 <= a->n - naxes, "sx_sample_fd_rows: axes outside [0, n)");
    const Geometry g = chain_geometry(a->C, a->n);
    SX_DISPATCH_LPR(a->n, hipLaunchKernelGGL((sample_fd_rows_kernel<LPR>), dim3(g.blocks, (unsigned)naxes), dim3(g.threads), 0,
                                             (hipStream_t)stream, *a, q, axis0, W))
    SX_LAUNCH_CHECK();
    return 0;
}

extern "C" int sx_sample_fd_gradient(const sx_sample_args *a, const double *fW, int axis0, int naxes, double *G,
                                     void *stream) {
    if (check_args(a, 0)) return -1;
    SX_REQUIRE(a->method == SX_SAMPLE_HMC && fW && G && a->fd_step != 0.0, "sx_sample_fd_gradient: hmc with fW, G and a step");
    SX_REQUIRE(axis0 >= 0 && naxes >= 1 && axis0 <= a->n - naxes, "sx_sample_fd_gradient: axes outside [0, n)");
    const Geometry g = chain_geometry(a->C, a->n);
    SX_DISPATCH_LPR(a->n, hipLaunchKernelGGL((sample_fd_gradient_kernel<LPR>), dim3(g.blocks), dim3(g.threads), 0,
                                             (hipStream_t)stream, *a, fW, axis0, naxes, G))
    SX_LAUNCH_CHECK();
    return 0;
}

extern "C" int sx_sample_decide(const sx_sample_args *a, int64_t it, const double *prop, const double *fprop,
                                const double *pmom, const double *k0, void *stream) {
    if (check_args(a, it)) return -1;
    SX_REQUIRE(prop && fprop, "sx_sample_decide: null proposal / value array");
    SX_REQUIRE(a->method == SX_SAMPLE_MCMC || it == 0 || (pmom && k0), "sx_sample_decide: hmc needs pmom and k0");
    const Geometry g = chain_geometry(a->C, a->n);
    SX_DISPATCH_LPR(a->n, hipLaunchKernelGGL((sample_decide_kernel<LPR>), dim3(g.blocks), dim3(g.threads), 0,
                                             (hipStream_t)stream, *a, it, prop, fprop, pmom, k0))
    SX_LAUNCH_CHECK();
    return 0;
}

// The adapting / thinning forms (sx_sample_adapt): the checks of the plain entry points, then check_adapt
extern "C" int sx_sample_propose_adapt(const sx_sample_args *a, const sx_sample_adapt *ad, int64_t it, double *prop,
                                       double *pmom, double *k0, void *stream) {
    if (check_args(a, it) || check_adapt(a, ad)) return -1;
    SX_REQUIRE(prop != nullptr, "sx_sample_propose_adapt: null proposal array");
    SX_REQUIRE(a->method == SX_SAMPLE_MCMC || it == 0 || (pmom && k0), "sx_sample_propose_adapt: hmc needs pmom and k0");
    const Geometry g = chain_geometry(a->C, a->n);
    SX_DISPATCH_LPR(a->n, hipLaunchKernelGGL((sample_propose_adapt_kernel<LPR>), dim3(g.blocks), dim3(g.threads), 0,
                                             (hipStream_t)stream, *a, *ad, it, prop, pmom, k0))
    SX_LAUNCH_CHECK();
    return 0;
}

extern "C" int sx_sample_leap_adapt(const sx_sample_args *a, const sx_sample_adapt *ad, double coef, int move, double *q,
                                    double *pmom, const double *G, void *stream) {
    if (check_args(a, 0) || check_adapt(a, ad)) return -1;
    SX_REQUIRE(a->method == SX_SAMPLE_HMC && q && pmom && G, "sx_sample_leap_adapt: hmc with q, pmom and G");
    const Geometry g = chain_geometry(a->C, a->n);
    SX_DISPATCH_LPR(a->n, hipLaunchKernelGGL((sample_leap_adapt_kernel<LPR>), dim3(g.blocks), dim3(g.threads), 0,
                                             (hipStream_t)stream, *a, *ad, coef, move, q, pmom, G))
    SX_LAUNCH_CHECK();
    return 0;
}

extern "C" int sx_sample_decide_adapt(const sx_sample_args *a, const sx_sample_adapt *ad, int64_t it, const double *prop,
                                      const double *fprop, const double *pmom, const double *k0, void *stream) {
    if (check_args(a, it) || check_adapt(a, ad)) return -1;
    SX_REQUIRE(prop && fprop, "sx_sample_decide_adapt: null proposal / value array");
    SX_REQUIRE(a->method == SX_SAMPLE_MCMC || it == 0 || (pmom && k0), "sx_sample_decide_adapt: hmc needs pmom and k0");
    const Geometry g = chain_geometry(a->C, a->n);
    SX_DISPATCH_LPR(a->n, hipLaunchKernelGGL((sample_decide_adapt_kernel<LPR>), dim3(g.blocks), dim3(g.threads), 0,
                                             (hipStream_t)stream, *a, *ad, it, prop, fprop, pmom, k0))
    SX_LAUNCH_CHECK();
    return 0;
}

extern "C" int sx_sample_decide_tempered(const sx_sample_args *a, int64_t it, const double *prop, const double *fprop,
                                         const double *beta, int K, int record, void *stream) {
    if (check_args(a, it)) return -1;
    SX_REQUIRE(prop && fprop && beta, "sx_sample_decide_tempered: null proposal / value / beta array");
    SX_REQUIRE(a->method == SX_SAMPLE_MCMC, "sx_sample_decide_tempered: mcmc only");
    SX_REQUIRE(K >= 2 && a->C % K == 0, "sx_sample_decide_tempered: C is ladders x K replicas, K >= 2");
    const Geometry g = chain_geometry(a->C, a->n);
    Enqueue q((hipStream_t)stream);
    SX_DISPATCH_LPR(a->n, return q.kernel(sample_decide_tempered_kernel<LPR>, dim3(g.blocks), dim3(g.threads), 0, *a, it, prop,
                                          fprop, beta, K, record))
    return -1;
}

extern "C" int sx_sample_swap(const sx_sample_args *a, int64_t it, int64_t j, const double *beta, int K, int64_t *nswap,
                              void *stream) {
    if (check_args(a, it)) return -1;
    SX_REQUIRE(beta && nswap, "sx_sample_swap: null beta / nswap array");
    SX_REQUIRE(a->method == SX_SAMPLE_MCMC, "sx_sample_swap: mcmc only");
    SX_REQUIRE(K >= 2 && a->C % K == 0 && it >= 1 && j >= 1, "sx_sample_swap: C is ladders x K replicas, K >= 2; it, j >= 1");
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
