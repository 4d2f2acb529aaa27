// Parallel tempering (replica exchange) for the Metropolis-Hastings chains: LADDERS of K device-resident replicas.
//
// Replica q = c K + k is rung k of ladder c and samples p^(beta[k]), beta[k] = 1 / T_k, 1 = T_0 < T_1 < ... < T_{K-1}: its
// proposal and acceptance test are mcmc_kernel's (sx_sample.hpp mcmc_propose / chain_decide, as the unfused kernels') with
// d = (fcur - fprop) * beta[k], its draws are keyed by q in the place of the chain index.  After sample `it` (it >= 1,
// it % swap_every == 0) the exchange event j = it / swap_every pairs neighbouring rungs -- odd j (0,1), (2,3), ..., even j
// (1,2), (3,4), ...; a rung without a partner sits out -- and a pair exchanges its STATES (X and fcur; the rungs stay where
// they are) when sx_sample.hpp tempered_swap says so.  Sample `it` of a replica is its state after the event; an arriving
// state is compared with the replica's best values as an accepted proposal is, and moves neither nacc nor nfeas.
//
// Layout: a workgroup of `rows` row groups carries floor(rows / K) WHOLE ladders in consecutive row slots, so a ladder never
// spans two workgroups and an exchange is two workgroup barriers and a row copy in LDS: no grid barrier, no atomics, no
// spin-wait, nothing passes between workgroups, one launch per run.  The rows left over in a workgroup and the rows past the
// last ladder idle: they own no LDS and do nothing but reach the barriers (the sample loop and the event test are uniform over
// the workgroup).  LDS per live row as mcmc_kernel: X[n] | U[gen_row_stride(n)].
//
// The exchange phase:  lane 0 of a row publishes fcur -> barrier -> both rows of a pair compute the same decision from the same
// inputs (no flag is passed) and a swapping row copies its partner's X into its OWN proposal area U, dead at that point ->
// barrier -> U -> X -> wave fence before the next proposal reads X.
//
// Only rung-0 rows write xall / funall, at ladder index c.  State that survives from launch to launch stays in
// sx_sample_args' per-chain arrays (now C K long) and in nswap: a run cut into launches is the same run, bit for bit.
#include "sx_enqueue.hpp"
#include "sx_host.hpp"
#include "sx_rowops.hpp"
#include "sx_sample.hpp"

namespace sx {
int make_plan_arg(int fun_id, int n, PlanArg *out);

namespace {

// what the rows of a workgroup may take of its LDS (gfx950: 160 KiB), the kernel's static array left aside
constexpr size_t kLdsPerWorkgroup = 160 * 1024 - kMaxRowsPerBlock * sizeof(double);

// The objectives whose mcmc_kernel runs 4 waves per SIMD (120 - 124 VGPRs at 16 / 32 lanes per row) keep that here: the ladder's
// few extra registers would otherwise cost the fourth wave (128 - 133 without the hint; with it 128, no scratch) -- which cost
// more than the exchanges themselves
template <int FUN, int LPR>
constexpr int tempered_min_waves() {
    return LPR < kWave && (FUN == SX_FUN_ROSENBROCK || FUN == SX_FUN_SPHERE || FUN == SX_FUN_STYBLINSKI_TANG) ? 4 : 1;
}

template <int FUN, int LPR>
__global__ __launch_bounds__(kMaxWavesPerBlock *kWave, (tempered_min_waves<FUN, LPR>())) void mcmc_tempered_kernel(const sx_sample_args a, const PlanArg plan,
                                                                                 const double *__restrict__ beta, int K,
                                                                                 int64_t swap_every, int64_t *__restrict__ nswap,
                                                                                 int64_t it0, int64_t it1) {
    extern __shared__ double lds[];
    __shared__ double sf[kMaxRowsPerBlock];  // the rows' current values, published for an exchange
    const RowIds<LPR> id(a.C);
    const int n = a.n, l = id.l, k = a.k;
    const int rows = (int)(blockDim.x >> 6) * RowIds<LPR>::RPW;
    const int per_wg = rows / K;  // whole ladders of this workgroup (the launch makes rows >= K)
    const int lad = id.slot / K, rung = id.slot - lad * K;
    // (32-bit: the launch checks C < 2^31)
    const int c = (int)blockIdx.x * per_wg + lad;  // the ladder
    const bool live = lad < per_wg && c < (int)(a.C / K);
    const int q = c * K + rung;  // the replica: the chain index of every draw and of the per-chain arrays
    const int rd = sample_row_doubles(kMcmc, n);
    double *X = lds + (size_t)id.slot * rd;  // (live rows only: slots [0, per_wg K))
    double *U = X + n;
    const int nblocks = (n + k - 1) / k;
    ChainState st;
    if (live) {
        if (it0 > 0) {
            st.load(a, q);
            for (int e = l; e < n; e += LPR) X[e] = a.cur[(int64_t)q * n + e];
        } else if (l == 0) {
            nswap[q] = 0;  // (counted in memory by this row alone: no register held across the objective)
        }
    }
    for (int64_t it = it0; it < it1; ++it) {
        if (live) {
            int j0 = 0, j1 = 0;
            if (it == 0) {
                for (int e = l; e < n; e += LPR) U[e] = initial_value<LPR>(a, q, e);
            } else {
                mcmc_block(it, n, k, nblocks, j0, j1);
                mcmc_propose<LPR>(
                    a, (uint32_t)q, it, X, l, j0, j1, [&](int e) { return chain_step<false>(a, 1.0, e); },
                    [&](int e, double v) { U[e] = v; });
            }
            const double fU = row_objective<FUN, LPR, 0, 0>(U, n, plan, l);
            bool xbest_changed = true;  // (sample 0)
            if (it == 0) {
                st.start(fU);
                for (int e = l; e < n; e += LPR) X[e] = U[e];
            } else {
                const bool feasible = !a.reject || row_in_box<LPR>(a, U, n, l);
                // (beta = 1.0 on the cold rung: mcmc_kernel's d, bit for bit)
                const Decision r = chain_decide(st, a, (uint32_t)q, it, true, feasible, (st.fcur - fU) * beta[rung], fU);
                if (r.accept)
                    for (int e = l + ((j0 - l + LPR - 1) / LPR) * LPR; e < j1; e += LPR) X[e] = U[e];
                xbest_changed = r.xbest_changed;
            }
            if (xbest_changed)  // (before the exchange: the state may leave this replica)
                for (int e = l; e < n; e += LPR) a.xbest[(int64_t)q * n + e] = X[e];
        }
        if (it >= 1 && it % swap_every == 0) {  // uniform over the workgroup
            if (live && l == 0) sf[id.slot] = st.fcur;
            __syncthreads();
            bool swap = false, lower = false;
            double fin = 0.0;
            if (live) {
                const int kl = tempered_pair(rung, K, it / swap_every);
                if (kl >= 0) {
                    lower = kl == rung;
                    const int sl = id.slot - rung + kl;  // the lower rung's row slot
                    const double fl = sf[sl], fu = sf[sl + 1];
                    swap = tempered_swap(fl, fu, beta[kl], beta[kl + 1], (uint32_t)(q - rung + kl), (uint32_t)it, a.key0, a.key1);
                    if (swap) {
                        fin = lower ? fu : fl;
                        const double *PX = lds + (size_t)(lower ? sl + 1 : sl) * rd;  // the partner's X
                        for (int e = l; e < n; e += LPR) U[e] = PX[e];
                    }
                }
            }
            __syncthreads();
            if (swap) {
                bool acc_best;
                st.arrive(fin, it, acc_best);
                if (lower && l == 0) nswap[q] += 1;
                for (int e = l; e < n; e += LPR) X[e] = U[e];
                if (acc_best)
                    for (int e = l; e < n; e += LPR) a.xbest[(int64_t)q * n + e] = U[e];
            }
            lds_wave_fence();  // X complete before the next proposal reads it
        }
        if (live && rung == 0 && a.xall != nullptr) {
            double *dst = a.xall + ((int64_t)c * a.maxiter + it) * n;
            for (int e = l; e < n; e += LPR) st_stream(dst + e, X[e]);
            if (l == 0) st_stream(a.funall + (int64_t)c * a.maxiter + it, st.fcur);
        }
    }
    if (live) {
        for (int e = l; e < n; e += LPR) a.cur[(int64_t)q * n + e] = X[e];
        if (l == 0) st.store(a, q);
    }
}

using tempered_kernel_t = void (*)(const sx_sample_args, const PlanArg, const double *, int, int64_t, int64_t *, int64_t, int64_t);

// rows a workgroup can hold at all: the row kernels' caps
inline int max_rows(int n) {
    const int cap = kMaxWavesPerBlock * (kWave / lanes_per_row(n));
    return cap < kMaxRowsPerBlock ? cap : kMaxRowsPerBlock;
}

}  // namespace
}  // namespace sx

using namespace sx;

extern "C" int sx_sample_tempered_max_rungs(int n) {
    if (n < 1 || n > kWideFrom) return -1;
    const int fit = (int)(kLdsPerWorkgroup / (sizeof(double) * sample_row_doubles(kMcmc, n)));
    return fit < max_rows(n) ? fit : max_rows(n);
}

extern "C" int sx_sample_tempered_run(const sx_sample_args *a, const double *beta, int K, int64_t swap_every, int64_t *nswap,
                                      int64_t it0, int64_t steps, void *stream) {
    const char *who = "sx_sample_tempered_run";
    SX_SAMPLE_REQUIRE(a != nullptr && beta != nullptr && nswap != nullptr, "null args / beta / nswap");
    if (check_sample_args(who, a, it0, steps, true, false)) return -1;
    SX_SAMPLE_REQUIRE(a->method == SX_SAMPLE_MCMC, "mcmc only");
    SX_SAMPLE_REQUIRE(K >= 2 && K <= sx_sample_tempered_max_rungs(a->n), "K outside [2, sx_sample_tempered_max_rungs(n)]");
    SX_SAMPLE_REQUIRE(a->C % K == 0, "C is ladders x K replicas");
    SX_SAMPLE_REQUIRE(swap_every >= 1, "swap_every < 1");
    if (steps == 0) return 0;
    PlanArg plan;
    if (make_plan_arg(a->fun_id, a->n, &plan)) return -1;
    tempered_kernel_t kern = nullptr;
    SX_DISPATCH_LPR(a->n, SX_DISPATCH_FUN(a->fun_id, (kern = mcmc_tempered_kernel<FUN, LPR>)))
    const int rpw = kWave / lanes_per_row(a->n);
    int waves = sample_waves(kMcmc, a->n);
    while (waves * rpw < K) waves *= 2;  // (K <= max_rows(n): ends at kMaxWavesPerBlock or before)
    const int per_wg = waves * rpw / K;
    const int64_t ladders = a->C / K;
    const size_t lds = (size_t)per_wg * K * sample_row_doubles(kMcmc, a->n) * sizeof(double);
    SX_SAMPLE_REQUIRE(lds <= kLdsPerWorkgroup, "the ladders of a workgroup do not fit its LDS");
    if (lds > 64 * 1024)  // more than the default limit (gfx950: 160 KiB per workgroup)
        SX_HIP(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    Enqueue q((hipStream_t)stream);
    return q.kernel(kern, dim3((unsigned)((ladders + per_wg - 1) / per_wg)), dim3(waves * kWave), lds, *a, plan, beta, K,
                    swap_every, nswap, it0, it0 + steps);
}
