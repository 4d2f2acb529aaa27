// Samplers (stochopy/sample): Metropolis-Hastings and Hamiltonian Monte-Carlo with many independent chains.
//
// A Markov chain is sequential, independent chains never talk to each other: one row group (lanes_per_row(n) lanes)
// carries ONE chain for the whole launch.  The chain's rows -- current sample, proposal / position, momentum and the two
// finite-difference copies -- live in that row group's slice of LDS, its scalars (current value, best values, counts)
// in registers; there is no workgroup barrier, no grid barrier and no exchange.  A launch advances every chain by
// `it1 - it0` samples and writes row i of xall / funall with streaming stores as it goes.  State that has to survive
// from launch to launch (a run with a callback is one launch per sample) round-trips through sx_sample_args' per-chain
// arrays unchanged, so cutting a run into launches does not change a bit of it.
//
// Draws: SX_RNG_HOST reads the reference's own stream from memory (normals, log of the acceptance uniform: the order
// does not depend on the data as long as nothing is rejected for feasibility); SX_RNG_PHILOX keys every draw by
// (slot, chain, sample, purpose) -- sx_device.hpp kPurposeSample* -- so a chain depends on its index and the key only.
#include "sx_host.hpp"
#include "sx_rowops.hpp"
#include "sx_sample.hpp"

namespace sx {
int make_plan_arg(int fun_id, int n, PlanArg *out);

namespace {

// f(e, dF/dx_e) for every element this lane owns; Q complete and fenced by the caller
template <int FUN, int LPR, class F>
__device__ __forceinline__ void grad_apply(const double *Q, int n, int l, F &&f) {
    using G = Grad<FUN>;
    double ra = 0.0, rb = G::BMUL ? 1.0 : 0.0;
    if constexpr (G::REDUCE) {
        for (int e = l; e < n; e += LPR) {
            double a, b;
            G::pre(Q[e], e, a, b);
            ra += a;
            rb = combine<G::BMUL>(rb, b);
        }
        ra = row_sum<LPR>(ra);
        rb = G::BMUL ? row_prod<LPR>(rb) : row_sum<LPR>(rb);
    }
    for (int e = l; e < n; e += LPR) {
        const double x = Q[e];
        const double xp = e > 0 ? Q[e - 1] : 0.0, xn = e < n - 1 ? Q[e + 1] : 0.0;
        f(e, G::elem(x, xp, xn, e, n, ra, rb));
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Metropolis-Hastings (mcmc/_mcmc.py:104-156).  Sample i perturbs block (i-1) mod ceil(n/k) of k consecutive variables
// (the last block is the shorter one when k does not divide n): randn(kb) * step, then rand() for the decision.
// LDS per chain: X[n] (current sample) | U[gen_row_stride(n)] (proposal, in the objective's layout).
// ---------------------------------------------------------------------------------------------------------------------
// ADAPT (sx_sample_adapt): the chain's multiplier of a.step adapts during the warm-up and xall / funall take the recorded
// rows only; without it `ad` is an empty struct that is never read, and the kernel is the plain one.
template <int FUN, int LPR, bool ADAPT>
__global__ __launch_bounds__(kMaxWavesPerBlock *kWave) void mcmc_kernel(const sx_sample_args a, const PlanArg plan,
                                                                        int64_t it0, int64_t it1, const AdaptArg<ADAPT> ad) {
    extern __shared__ double lds[];
    const RowIds<LPR> id(a.C);
    const int n = a.n, l = id.l, k = a.k;
    const int64_t c = id.rowc;
    double *X = lds + (size_t)id.slot * sample_row_doubles(kMcmc, n);
    double *U = X + n;
    const bool host = a.rng == SX_RNG_HOST;
    const int nblocks = (n + k - 1) / k;
    ChainState st;
    AdaptState as;
    if (it0 > 0) {
        st.load(a, c);
        if constexpr (ADAPT) as.load(ad, c);
        for (int e = l; e < n; e += LPR) X[e] = a.cur[c * n + e];
    }
    const auto step = [&](int e) {
        if constexpr (ADAPT)
            return as.s * a.step[e];
        else
            return a.step[e];
    };
    int64_t rec_next = 0, rec_row = 0;  // (ADAPT) the next recorded sample and its row: no division per sample
    if constexpr (ADAPT) adapt_first_record(ad, it0, rec_next, rec_row);
    for (int64_t it = it0; it < it1; ++it) {
        int j0 = 0, j1 = 0;
        if (it == 0) {
            for (int e = l; e < n; e += LPR) U[e] = initial_value<LPR>(a, c, e);
        } else {
            j0 = (int)((it - 1) % nblocks) * k;
            j1 = j0 + k < n ? j0 + k : n;
            for (int e0 = l; e0 < n; e0 += 2 * LPR) {  // element pairs (e0, e0 + LPR): one Box-Muller call
                const int e1 = e0 + LPR;
                const bool in0 = e0 >= j0 && e0 < j1, in1 = e1 >= j0 && e1 < j1;
                double z0 = 0.0, z1 = 0.0;
                if (host) {
                    if (in0) z0 = a.normals[(it - 1) * k + (e0 - j0)];
                    if (in1) z1 = a.normals[(it - 1) * k + (e1 - j0)];
                } else if (in0 || in1) {
                    philox_normal_pair<LPR>(e0, (uint32_t)c, (uint32_t)it, kPurposeSampleProposal, a.key0, a.key1, z0, z1);
                }
                const double v0 = X[e0];
                U[e0] = in0 ? v0 + z0 * step(e0) : v0;
                if (e1 < n) {
                    const double v1 = X[e1];
                    U[e1] = in1 ? v1 + z1 * step(e1) : v1;
                }
            }
        }
        // (an infeasible proposal is evaluated too and its value dropped: the rows of a wave stay in step)
        const double fU = row_objective<FUN, LPR, 0, 0>(U, n, plan, l);
        bool xbest_changed = false;
        if (it == 0) {
            st.start(fU);
            if constexpr (ADAPT) as.start();
            for (int e = l; e < n; e += LPR) X[e] = U[e];
            xbest_changed = true;  // x = xall[0] while nothing was accepted
        } else {
            const bool feasible = !a.reject || row_in_box<LPR>(a, U, n, l);
            bool accept = false;
            double dstat = 0.0;
            if (feasible) {
                st.nfeas += 1;
                const double logu = host ? a.logu[it] : philox_log_accept((uint32_t)c, (uint32_t)it, a.key0, a.key1);
                const double d = st.fcur - fU;
                accept = (d < 0.0 ? d : 0.0) > logu;  // Python's min(0.0, d): a NaN d gives 0.0
                dstat = d;
            }
            if (accept) {
                bool arg_best;
                st.accept(fU, it, xbest_changed, arg_best);
                for (int e = l + ((j0 - l + LPR - 1) / LPR) * LPR; e < j1; e += LPR) X[e] = U[e];
            }
            if constexpr (ADAPT) adapt_update(as, ad.warmup, ad.target, it, feasible, dstat, st.nacc);
        }
        if (id.active) {
            if constexpr (ADAPT) {
                if (a.xall != nullptr && it == rec_next) {
                    double *dst = a.xall + (c * ad.rec_rows + rec_row) * n;
                    for (int e = l; e < n; e += LPR) st_stream(dst + e, X[e]);
                    if (l == 0) st_stream(a.funall + c * ad.rec_rows + rec_row, st.fcur);
                }
            } else if (a.xall != nullptr) {
                double *dst = a.xall + (c * a.maxiter + it) * n;
                for (int e = l; e < n; e += LPR) st_stream(dst + e, X[e]);
                if (l == 0) st_stream(a.funall + c * a.maxiter + it, st.fcur);
            }
            if (xbest_changed)
                for (int e = l; e < n; e += LPR) a.xbest[c * n + e] = X[e];
        }
        if constexpr (ADAPT)
            if (it == rec_next) rec_next += ad.rec_every, rec_row += 1;
    }
    if (id.active) {
        for (int e = l; e < n; e += LPR) a.cur[c * n + e] = X[e];
        if (l == 0) {
            st.store(a, c);
            if constexpr (ADAPT) as.store(ad, c);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Hamiltonian Monte-Carlo (hmc/_hmc.py:135-185).  Per sample: momentum p = randn(n); nleap + 2 gradients and nleap + 1
// position steps (half momentum step, position step, nleap x (momentum step, position step), half momentum step);
// d = U0 - U + K0 - K; rand() for the decision.  U0 = fun(q0) is the current value (the reference evaluates it again).
// ANALYTIC: sx_device.hpp Grad<FUN>.  Finite differences (numerical_gradient, :215-231): x1 / x2 are copies of q whose
// component i is moved by -h / +h and moved BACK in place, so later components see the rounding of earlier ones.
// LDS per chain: X[n] current sample | Q[S] position | P[n] momentum | finite differences: X1[S] | X2[S]
// (S = gen_row_stride(n): the objective's layout).
// ---------------------------------------------------------------------------------------------------------------------
template <int FUN, int LPR, bool ANALYTIC, bool ADAPT>
__global__ __launch_bounds__(kMaxWavesPerBlock *kWave) void hmc_kernel(const sx_sample_args a, const PlanArg plan,
                                                                       int64_t it0, int64_t it1, const AdaptArg<ADAPT> ad) {
    extern __shared__ double lds[];
    const RowIds<LPR> id(a.C);
    const int n = a.n, l = id.l, S = gen_row_stride(n);
    const int64_t c = id.rowc;
    double *X = lds + (size_t)id.slot * sample_row_doubles(ANALYTIC ? kHmcAnalytic : kHmcFd, n);
    double *Q = X + n;
    double *Pm = Q + S;
    double *X1 = Pm + n, *X2 = X1 + S;  // (finite differences only)
    const bool host = a.rng == SX_RNG_HOST;
    const double h = a.fd_step;
    ChainState st;
    AdaptState as;
    if (it0 > 0) {
        st.load(a, c);
        if constexpr (ADAPT) as.load(ad, c);
        for (int e = l; e < n; e += LPR) X[e] = a.cur[c * n + e];
    }
    const auto step = [&](int e) {
        if constexpr (ADAPT)
            return as.s * a.step[e];
        else
            return a.step[e];
    };
    int64_t rec_next = 0, rec_row = 0;  // (ADAPT) the next recorded sample and its row: no division per sample
    if constexpr (ADAPT) adapt_first_record(ad, it0, rec_next, rec_row);
    for (int64_t it = it0; it < it1; ++it) {
        double K0 = 0.0, K = 0.0;
        if (it == 0) {
            for (int e = l; e < n; e += LPR) Q[e] = initial_value<LPR>(a, c, e);
        } else {
            double s = 0.0;
            for (int e0 = l; e0 < n; e0 += 2 * LPR) {
                const int e1 = e0 + LPR;
                double z0 = 0.0, z1 = 0.0;
                if (host) {
                    z0 = a.normals[(it - 1) * n + e0];
                    if (e1 < n) z1 = a.normals[(it - 1) * n + e1];
                } else {
                    philox_normal_pair<LPR>(e0, (uint32_t)c, (uint32_t)it, kPurposeSampleMomentum, a.key0, a.key1, z0, z1);
                }
                Q[e0] = X[e0];
                Pm[e0] = z0;
                s += z0 * z0;
                if (e1 < n) {
                    Q[e1] = X[e1];
                    Pm[e1] = z1;
                    s += z1 * z1;
                }
            }
            K0 = 0.5 * row_sum<LPR>(s);
#pragma unroll 1
            for (int g = 0; g <= a.nleap + 1; ++g) {
                const double coef = (g == 0 || g == a.nleap + 1) ? 0.5 : 1.0;
                lds_wave_fence();  // Q complete
                if constexpr (ANALYTIC) {
                    grad_apply<FUN, LPR>(Q, n, l, [&](int e, double gv) { Pm[e] = Pm[e] - (coef * step(e)) * gv; });
                } else {
                    for (int e = l; e < n; e += LPR) X1[e] = X2[e] = Q[e];
#pragma unroll 1
                    for (int i = 0; i < n; ++i) {
                        const bool own = (i & (LPR - 1)) == l;
                        if (own) {
                            X1[i] = X1[i] - h;
                            X2[i] = X2[i] + h;
                        }
                        double fv[2];
#pragma unroll 1
                        for (int w = 0; w < 2; ++w) fv[w] = row_objective<FUN, LPR, 0, 0>(w ? X1 : X2, n, plan, l);
                        const double gv = (0.5 * (fv[0] - fv[1])) / h;
                        if (own) {
                            Pm[i] = Pm[i] - (coef * step(i)) * gv;
                            X1[i] = X1[i] + h;
                            X2[i] = X2[i] - h;
                        }
                    }
                }
                if (g <= a.nleap)
                    for (int e = l; e < n; e += LPR) Q[e] = Q[e] + step(e) * Pm[e];
            }
            s = 0.0;
            for (int e = l; e < n; e += LPR) s += Pm[e] * Pm[e];
            K = 0.5 * row_sum<LPR>(s);
        }
        const double fQ = row_objective<FUN, LPR, 0, 0>(Q, n, plan, l);
        bool xbest_changed = false;
        if (it == 0) {
            st.start(fQ);
            if constexpr (ADAPT) as.start();
            for (int e = l; e < n; e += LPR) X[e] = Q[e];
            xbest_changed = true;
        } else {
            const bool feasible = !a.reject || row_in_box<LPR>(a, Q, n, l);
            bool accept = false;
            double dstat = 0.0;
            if (feasible) {
                st.nfeas += 1;
                const double logu = host ? a.logu[it] : philox_log_accept((uint32_t)c, (uint32_t)it, a.key0, a.key1);
                const double d = ((st.fcur - fQ) + K0) - K;
                accept = (d < 0.0 ? d : 0.0) > logu;
                dstat = d;
            }
            if (accept) {
                bool acc_best;
                st.accept(fQ, it, acc_best, xbest_changed);
                for (int e = l; e < n; e += LPR) X[e] = Q[e];
            }
            if constexpr (ADAPT) adapt_update(as, ad.warmup, ad.target, it, feasible, dstat, st.nacc);
        }
        if (id.active) {
            if constexpr (ADAPT) {
                if (a.xall != nullptr && it == rec_next) {
                    double *dst = a.xall + (c * ad.rec_rows + rec_row) * n;
                    for (int e = l; e < n; e += LPR) st_stream(dst + e, X[e]);
                    if (l == 0) st_stream(a.funall + c * ad.rec_rows + rec_row, st.fcur);
                }
            } else if (a.xall != nullptr) {
                double *dst = a.xall + (c * a.maxiter + it) * n;
                for (int e = l; e < n; e += LPR) st_stream(dst + e, X[e]);
                if (l == 0) st_stream(a.funall + c * a.maxiter + it, st.fcur);
            }
            if (xbest_changed)
                for (int e = l; e < n; e += LPR) a.xbest[c * n + e] = X[e];
        }
        if constexpr (ADAPT)
            if (it == rec_next) rec_next += ad.rec_every, rec_row += 1;
    }
    if (id.active) {
        for (int e = l; e < n; e += LPR) a.cur[c * n + e] = X[e];
        if (l == 0) {
            st.store(a, c);
            if constexpr (ADAPT) as.store(ad, c);
        }
    }
}

template <int FUN, int LPR>
__global__ __launch_bounds__(kMaxWavesPerBlock *kWave) void gradient_kernel(const double *__restrict__ Xg, int64_t P, int n,
                                                                            double *__restrict__ G) {
    extern __shared__ double lds[];
    const RowIds<LPR> id(P);
    const int l = id.l;
    double *Q = lds + (size_t)id.slot * n;
    for (int e = l; e < n; e += LPR) Q[e] = Xg[id.rowc * n + e];
    lds_wave_fence();
    const bool active = id.active;
    double *g = G + id.rowc * n;
    grad_apply<FUN, LPR>(Q, n, l, [&](int e, double gv) {
        if (active) g[e] = gv;
    });
}

template <bool ADAPT>
using sample_kernel_t = void (*)(const sx_sample_args, const PlanArg, int64_t, int64_t, const AdaptArg<ADAPT>);
using gradient_kernel_t = void (*)(const double *, int64_t, int, double *);

template <int FUN, int LPR, bool ADAPT>
sample_kernel_t<ADAPT> pick_variant(int variant) {
    return variant == kMcmc    ? mcmc_kernel<FUN, LPR, ADAPT>
           : variant == kHmcFd ? hmc_kernel<FUN, LPR, false, ADAPT>
                               : hmc_kernel<FUN, LPR, true, ADAPT>;
}
template <int LPR, bool ADAPT>
sample_kernel_t<ADAPT> pick_sample(int fun_id, int variant) {
    switch (fun_id) {
        case SX_FUN_ACKLEY: return pick_variant<SX_FUN_ACKLEY, LPR, ADAPT>(variant);
        case SX_FUN_GRIEWANK: return pick_variant<SX_FUN_GRIEWANK, LPR, ADAPT>(variant);
        case SX_FUN_QUARTIC: return pick_variant<SX_FUN_QUARTIC, LPR, ADAPT>(variant);
        case SX_FUN_RASTRIGIN: return pick_variant<SX_FUN_RASTRIGIN, LPR, ADAPT>(variant);
        case SX_FUN_ROSENBROCK: return pick_variant<SX_FUN_ROSENBROCK, LPR, ADAPT>(variant);
        case SX_FUN_SPHERE: return pick_variant<SX_FUN_SPHERE, LPR, ADAPT>(variant);
        default: return pick_variant<SX_FUN_STYBLINSKI_TANG, LPR, ADAPT>(variant);
    }
}
template <int LPR>
gradient_kernel_t pick_gradient(int fun_id) {
    switch (fun_id) {
        case SX_FUN_ACKLEY: return gradient_kernel<SX_FUN_ACKLEY, LPR>;
        case SX_FUN_GRIEWANK: return gradient_kernel<SX_FUN_GRIEWANK, LPR>;
        case SX_FUN_QUARTIC: return gradient_kernel<SX_FUN_QUARTIC, LPR>;
        case SX_FUN_RASTRIGIN: return gradient_kernel<SX_FUN_RASTRIGIN, LPR>;
        case SX_FUN_ROSENBROCK: return gradient_kernel<SX_FUN_ROSENBROCK, LPR>;
        case SX_FUN_SPHERE: return gradient_kernel<SX_FUN_SPHERE, LPR>;
        default: return gradient_kernel<SX_FUN_STYBLINSKI_TANG, LPR>;
    }
}

int variant_of(int method, int jac) { return method == SX_SAMPLE_MCMC ? kMcmc : jac == SX_JAC_ANALYTIC ? kHmcAnalytic : kHmcFd; }

}  // namespace
}  // namespace sx

using namespace sx;

extern "C" int sx_sample_chains_per_workgroup(int method, int jac, int n) {
    if (n < 1 || n > kWideFrom) return -1;
    return sample_waves(variant_of(method, jac), n) * (kWave / lanes_per_row(n));
}

namespace {
int check_run_args(const sx_sample_args *a, int64_t it0, int64_t steps) {
    SX_REQUIRE(a != nullptr, "sx_sample_run: null args");
    SX_REQUIRE(a->cur && a->fcur && a->facc && a->fmin && a->xbest && a->iacc && a->imin && a->nacc && a->nfeas,
               "sx_sample_run: null state pointer");
    SX_REQUIRE(a->lower && a->upper && a->step, "sx_sample_run: bounds / step missing");
    SX_REQUIRE(a->C >= 1 && a->C < (int64_t)1 << 31 && a->n >= 1 && a->n <= kWideFrom, "sx_sample_run: bad shape");
    SX_REQUIRE(a->fun_id >= 0 && a->fun_id < SX_FUN_COUNT, "sx_sample_run: unknown objective");
    SX_REQUIRE(a->method == SX_SAMPLE_MCMC || a->method == SX_SAMPLE_HMC, "sx_sample_run: unknown method");
    SX_REQUIRE(a->jac == SX_JAC_FINITE_DIFF || a->jac == SX_JAC_ANALYTIC, "sx_sample_run: unknown gradient mode");
    SX_REQUIRE(a->rng == SX_RNG_HOST || a->rng == SX_RNG_PHILOX, "sx_sample_run: unknown rng mode");
    SX_REQUIRE(a->maxiter >= 1 && a->maxiter < (int64_t)1 << 31 && it0 >= 0 && steps >= 0 && it0 + steps <= a->maxiter,
               "sx_sample_run: samples outside [0, maxiter)");
    SX_REQUIRE(a->rng != SX_RNG_HOST || (a->C == 1 && a->x0 && !a->reject && (a->maxiter == 1 || (a->normals && a->logu))),
               "sx_sample_run: host draws serve one chain without feasibility rejection, and need x0, normals and logu");
    SX_REQUIRE((a->xall == nullptr) == (a->funall == nullptr), "sx_sample_run: xall and funall go together");
    SX_REQUIRE(a->x0 == nullptr || a->x0_stride == 0 || a->x0_stride >= a->n, "sx_sample_run: bad x0 stride");
    if (a->method == SX_SAMPLE_MCMC)
        SX_REQUIRE(a->k >= 1 && a->k <= a->n, "sx_sample_run: block length outside [1, n]");
    else
        SX_REQUIRE(a->nleap >= 1 && (a->jac == SX_JAC_ANALYTIC || a->fd_step != 0.0), "sx_sample_run: bad nleap / step");
    return 0;
}
}  // namespace

extern "C" int sx_sample_run(const sx_sample_args *a, int64_t it0, int64_t steps, void *stream) {
    if (check_run_args(a, it0, steps)) return -1;
    if (steps == 0) return 0;
    PlanArg plan;
    if (make_plan_arg(a->fun_id, a->n, &plan)) return -1;
    const int variant = variant_of(a->method, a->jac);
    sample_kernel_t<false> kern = nullptr;
    SX_DISPATCH_LPR(a->n, kern = (pick_sample<LPR, false>(a->fun_id, variant)))
    const int waves = sample_waves(variant, a->n);
    const int chains = waves * (kWave / lanes_per_row(a->n));
    const size_t lds = (size_t)chains * sample_row_doubles(variant, a->n) * sizeof(double);
    if (lds > 64 * 1024)  // one wave's chains need more than the default limit (gfx950: 160 KiB per workgroup)
        SX_HIP(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kern, dim3((unsigned)((a->C + chains - 1) / chains)), dim3(waves * kWave), lds, (hipStream_t)stream,
                       *a, plan, it0, it0 + steps, NoAdapt{});
    SX_LAUNCH_CHECK();
    return 0;
}

extern "C" int sx_sample_adapt_bytes(void) { return (int)sizeof(sx_sample_adapt); }

// sx_sample_run with the adapting / thinning kernels (the same geometry and LDS)
extern "C" int sx_sample_run_adapt(const sx_sample_args *a, const sx_sample_adapt *ad, int64_t it0, int64_t steps,
                                   void *stream) {
    if (check_run_args(a, it0, steps) || check_adapt(a, ad)) return -1;
    if (steps == 0) return 0;
    PlanArg plan;
    if (make_plan_arg(a->fun_id, a->n, &plan)) return -1;
    const int variant = variant_of(a->method, a->jac);
    sample_kernel_t<true> kern = nullptr;
    SX_DISPATCH_LPR(a->n, kern = (pick_sample<LPR, true>(a->fun_id, variant)))
    const int waves = sample_waves(variant, a->n);
    const int chains = waves * (kWave / lanes_per_row(a->n));
    const size_t lds = (size_t)chains * sample_row_doubles(variant, a->n) * sizeof(double);
    if (lds > 64 * 1024)
        SX_HIP(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kern, dim3((unsigned)((a->C + chains - 1) / chains)), dim3(waves * kWave), lds, (hipStream_t)stream,
                       *a, plan, it0, it0 + steps, *ad);
    SX_LAUNCH_CHECK();
    return 0;
}

extern "C" int sx_sample_gradient(int fun_id, const double *X, int64_t P, int n, double *G, void *stream) {
    SX_REQUIRE(X && G && P >= 1 && n >= 1 && n <= kWideFrom, "sx_sample_gradient: bad arguments");
    SX_REQUIRE(fun_id >= 0 && fun_id < SX_FUN_COUNT, "sx_sample_gradient: unknown objective");
    gradient_kernel_t kern = nullptr;
    SX_DISPATCH_LPR(n, kern = pick_gradient<LPR>(fun_id))
    const int rpw = kWave / lanes_per_row(n);
    int waves = 1;
    while (2 * waves <= kMaxWavesPerBlock && 2 * waves * rpw <= kMaxRowsPerBlock && 2 * waves * rpw * n * 8 <= 64 * 1024) waves *= 2;
    const int rows = waves * rpw;
    hipLaunchKernelGGL(kern, dim3((unsigned)((P + rows - 1) / rows)), dim3(waves * kWave), (size_t)rows * n * sizeof(double),
                       (hipStream_t)stream, X, P, n, G);
    SX_LAUNCH_CHECK();
    return 0;
}
