// The resident chain kernels of the samplers (mcmc_kernel, hmc_kernel) and their launch, as templates: sx_sample.hip instantiates
// the plain and the adapting form, sx_sample_metric.hip the form with per-axis scales -- three forms in one translation unit
// compile for 94 s on one core, longer than the rest of the library on eight.  The file comment of sx_sample.hip describes them.
#pragma once
#include "sx_enqueue.hpp"
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
// METRIC (sx_sample_metric, with ADAPT): per-axis scales too -- the row gains EFF[n], the chain's m * step, behind the others;
// `ad` is then MetricAdapt.  A third instantiation: the other two keep their code.
template <int FUN, int LPR, bool ADAPT, bool METRIC = false>
__global__ __launch_bounds__(kMaxWavesPerBlock *kWave) void mcmc_kernel(const sx_sample_args a, const PlanArg plan,
                                                                        int64_t it0, int64_t it1,
                                                                        const AdaptArg<ADAPT, METRIC> ad) {
    extern __shared__ double lds[];
    const RowIds<LPR> id(a.C);
    const int n = a.n, l = id.l, k = a.k;
    const int64_t c = id.rowc;
    double *X = lds + (size_t)id.slot * sample_row_doubles(kMcmc, n, METRIC);
    double *U = X + n;
    double *EFF = X + sample_row_doubles(kMcmc, n);  // (METRIC only)
    double sbase = 1.0;                              // (METRIC only)
    const bool host = a.rng == SX_RNG_HOST;
    const int nblocks = (n + k - 1) / k;
    ChainState st;
    AdaptState as;
    if (it0 > 0) {
        st.load(a, c);
        if constexpr (ADAPT) as.load(ad, c);
        for (int e = l; e < n; e += LPR) X[e] = a.cur[c * n + e];
        if constexpr (METRIC) {
            sbase = metric_load_sbase(ad.mt, c);
            for (int e = l; e < n; e += LPR) EFF[e] = metric_eff(a, ad.mt, c, e);
        }
    }
    const auto step = [&](int e) {
        if constexpr (METRIC)
            return as.s * EFF[e];
        else if constexpr (ADAPT)
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
            if constexpr (METRIC) {
                metric_start<LPR>(a, ad.mt, c, l, id.active, sbase);
                for (int e = l; e < n; e += LPR) EFF[e] = 1.0 * a.step[e];
            }
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
            if constexpr (METRIC)  // (each lane reads back the elements of X and EFF it wrote itself)
                metric_update<LPR>(
                    a, ad, as, sbase, c, l, id.active, it, feasible, dstat, st.nacc, [&](int e) { return X[e]; },
                    [&](int e, double v) { EFF[e] = v; });
            else if constexpr (ADAPT)
                adapt_update(as, ad.warmup, ad.target, it, feasible, dstat, st.nacc);
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
template <int FUN, int LPR, bool ANALYTIC, bool ADAPT, bool METRIC = false>
__global__ __launch_bounds__(kMaxWavesPerBlock *kWave) void hmc_kernel(const sx_sample_args a, const PlanArg plan,
                                                                       int64_t it0, int64_t it1,
                                                                       const AdaptArg<ADAPT, METRIC> ad) {
    extern __shared__ double lds[];
    const RowIds<LPR> id(a.C);
    const int n = a.n, l = id.l, S = gen_row_stride(n);
    const int64_t c = id.rowc;
    double *X = lds + (size_t)id.slot * sample_row_doubles(ANALYTIC ? kHmcAnalytic : kHmcFd, n, METRIC);
    double *EFF = X + sample_row_doubles(ANALYTIC ? kHmcAnalytic : kHmcFd, n);  // (METRIC only)
    double sbase = 1.0;                                                         // (METRIC only)
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
        if constexpr (METRIC) {
            sbase = metric_load_sbase(ad.mt, c);
            for (int e = l; e < n; e += LPR) EFF[e] = metric_eff(a, ad.mt, c, e);
        }
    }
    const auto step = [&](int e) {
        if constexpr (METRIC)
            return as.s * EFF[e];
        else if constexpr (ADAPT)
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
            if constexpr (METRIC) {
                metric_start<LPR>(a, ad.mt, c, l, id.active, sbase);
                for (int e = l; e < n; e += LPR) EFF[e] = 1.0 * a.step[e];
            }
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
            if constexpr (METRIC)  // (each lane reads back the elements of X and EFF it wrote itself)
                metric_update<LPR>(
                    a, ad, as, sbase, c, l, id.active, it, feasible, dstat, st.nacc, [&](int e) { return X[e]; },
                    [&](int e, double v) { EFF[e] = v; });
            else if constexpr (ADAPT)
                adapt_update(as, ad.warmup, ad.target, it, feasible, dstat, st.nacc);
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

template <bool ADAPT, bool METRIC = false>
using sample_kernel_t = void (*)(const sx_sample_args, const PlanArg, int64_t, int64_t, const AdaptArg<ADAPT, METRIC>);

template <int FUN, int LPR, bool ADAPT, bool METRIC>
sample_kernel_t<ADAPT, METRIC> pick_variant(int variant) {
    return variant == kMcmc    ? mcmc_kernel<FUN, LPR, ADAPT, METRIC>
           : variant == kHmcFd ? hmc_kernel<FUN, LPR, false, ADAPT, METRIC>
                               : hmc_kernel<FUN, LPR, true, ADAPT, METRIC>;
}

int variant_of(int method, int jac) { return method == SX_SAMPLE_MCMC ? kMcmc : jac == SX_JAC_ANALYTIC ? kHmcAnalytic : kHmcFd; }

// sx_sample_run, its adapting / thinning form and the one with per-axis scales: the same geometry, the LDS by the form's row
template <bool ADAPT, bool METRIC = false>
int run_chains(const char *who, const sx_sample_args *a, const sx_sample_adapt *ad, const sx_sample_metric *mt, int64_t it0,
               int64_t steps, void *stream) {
    if (check_sample_args(who, a, it0, steps, true, true) || (ADAPT && check_adapt(a, ad)) || (METRIC && check_metric(ad, mt)))
        return -1;
    if (steps == 0) return 0;
    PlanArg plan;
    if (make_plan_arg(a->fun_id, a->n, &plan)) return -1;
    const int variant = variant_of(a->method, a->jac);
    sample_kernel_t<ADAPT, METRIC> kern = nullptr;
    SX_DISPATCH_LPR(a->n, SX_DISPATCH_FUN(a->fun_id, (kern = pick_variant<FUN, LPR, ADAPT, METRIC>(variant))))
    const int waves = sample_waves(variant, a->n, METRIC);
    const int chains = waves * (kWave / lanes_per_row(a->n));
    const size_t lds = (size_t)chains * sample_row_doubles(variant, a->n, METRIC) * sizeof(double);
    SX_SAMPLE_REQUIRE(lds <= 160 * 1024, "one wave's chains do not fit the 160 KiB of LDS of a workgroup");
    if (lds > 64 * 1024)  // one wave's chains need more than the default limit (gfx950: 160 KiB per workgroup)
        SX_HIP(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    return Enqueue((hipStream_t)stream)
        .kernel(kern, dim3((unsigned)((a->C + chains - 1) / chains)), dim3(waves * kWave), lds, *a, plan, it0, it0 + steps,
                adapt_arg<ADAPT, METRIC>(ad, mt));
}

}  // namespace
}  // namespace sx
