// Tempered sequential Monte Carlo (method="smc"; include/stochopy_hip.h states the rule): C populations of P particles walk
// from the uniform prior on the box (beta = 0) to the target exp(-fun) (beta = 1) through stages
//   stage kernel    one workgroup of 1 024 threads per population, its P values in LDS: the previous stage's acceptance ratio
//                   and the next scale, the next beta (52 halvings on the effective sample size), the evidence, the running
//                   sums of the weights (which take the values' place in LDS) and the systematic resampling -> anc
//   gather kernel   rows through anc into the other buffer, and from them the step of every axis (two-pass deviation)
//   mutation kernel one row group per particle, X | U in LDS for the M Metropolis steps, as mcmc_kernel; the step of a
//                   particle is sx_sample.hpp's (mcmc_propose on all variables, row_in_box, chain_decide with d times beta)
// and, around a caller's objective, the mutation step cut at the objective: propose kernel -> objective -> decide kernel.
// Nothing passes between workgroups: no grid barrier, no atomics, no spin-wait.  A population that has ended is frozen: its
// workgroup leaves the stage kernel at once (every thread on the same word of its record), its rows store nothing.
//
// The population's record, state[c][8] (doubles; the integers among them are exact):
//   [0] status (1 running, 0 reached beta = 1, -1 maxiter stages with beta < 1, -2 no finite value / a value of -inf)
//   [1] beta_s   [2] log Z so far   [3] ESS(beta_s) / P   [4] scale_s   [5] r_{s-1}, the last acceptance ratio known
//   [6] s, the stages done (the mutation of stage s runs the populations whose [6] is s)   [7] the accepted steps behind [5]
//
// No counterpart in the reference.
#include "sx_enqueue.hpp"
#include "sx_host.hpp"
#include "sx_rowops.hpp"
#include "sx_sample.hpp"

namespace sx {
int make_plan_arg(int fun_id, int n, PlanArg *out);
}
using namespace sx;

namespace {

constexpr int kSmcThreads = 1024, kSmcWaves = kSmcThreads / kWave;
constexpr int kSmcMaxParticles = 16384;  // 128 KiB of values / running sums in the 160 KiB of one workgroup
constexpr int kSmcHalvings = 52;
constexpr int kGatherAxes = 16, kGatherRows = 16;  // the gather kernel's 256 threads: 16 axes x 16 particles at a time
enum { kStStatus = 0, kStBeta, kStLogZ, kStEss, kStScale, kStAccept, kStStages, kStCount, kStWords };
constexpr double kSmcRunning = 1.0;
constexpr double kHuge = __builtin_huge_val();

// what sx_sample.hpp's step of a chain reads of its arguments: the row length, the box and the key
__device__ __forceinline__ sx_sample_args chain_view(const sx_smc_args &a) {
    sx_sample_args v = {};
    v.lower = a.lower, v.upper = a.upper;
    v.C = a.C * a.P;
    v.n = a.n, v.key0 = a.key0, v.key1 = a.key1;
    return v;
}

__device__ __forceinline__ void start_record(const sx_smc_args &a, int64_t c) {
    double *st = a.state + c * kStWords;
    for (int k = 0; k < kStWords; ++k) st[k] = 0.0;
    st[kStStatus] = kSmcRunning;
    st[kStScale] = a.scale;
}

// ---------------------------------------------------------------------------------------------------------------------
// The stage kernel.  Particle i of the population belongs to thread i / K, K = ceil(P / 1024): every thread owns K consecutive
// particles (the last ones fewer, or none).  A SUM over the population is formed as
//   thread: 0.0 + its terms in index order;  wave: v += v[lane ^ 1], ^ 2, ... ^ 32;  workgroup: 0.0 + the 16 waves' sums in order
// by thread 0, which publishes it -- and the decision taken from it -- in LDS: every thread takes the same branch from that
// one word, and reaches every barrier the same number of times.
// ---------------------------------------------------------------------------------------------------------------------
struct SmcShared {
    double part[2][kSmcWaves];
    double pub[3];
};

template <class T>
__device__ __forceinline__ T wave_xor_sum(T v) {
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) v += __shfl_xor(v, off, kWave);
    return v;
}

// (s0, s1) <- the sums of (v0, v1); pub[2] <- whether s0^2 / s1 >= thr.  Two barriers.
__device__ __forceinline__ bool block_sums(SmcShared &sh, double v0, double v1, double thr, double &s0, double &s1) {
    const int wave = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63);
    v0 = wave_xor_sum(v0), v1 = wave_xor_sum(v1);
    if (lane == 0) sh.part[0][wave] = v0, sh.part[1][wave] = v1;
    __syncthreads();
    if (threadIdx.x == 0) {
        double a = 0.0, b = 0.0;
        for (int w = 0; w < kSmcWaves; ++w) a += sh.part[0][w], b += sh.part[1][w];
        sh.pub[0] = a, sh.pub[1] = b, sh.pub[2] = (a * a) / b >= thr ? 1.0 : 0.0;
    }
    __syncthreads();
    s0 = sh.pub[0], s1 = sh.pub[1];
    return sh.pub[2] != 0.0;
}
__device__ __forceinline__ double block_min(SmcShared &sh, double v) {
    const int wave = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63);
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) v = fmin(v, __shfl_xor(v, off, kWave));
    if (lane == 0) sh.part[0][wave] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        double m = sh.part[0][0];
        for (int w = 1; w < kSmcWaves; ++w) m = fmin(m, sh.part[0][w]);
        sh.pub[0] = m;
    }
    __syncthreads();
    return sh.pub[0];
}

// w_i(beta) = exp(-(beta - beta_{s-1}) (f_i - f_min)); 0 where f_i is NaN or +inf
__device__ __forceinline__ double smc_weight(double f, double db, double fmin) {
    return (f == f && f < kHuge) ? exp(-(db * (f - fmin))) : 0.0;
}

// sum w, sum w^2 at beta_{s-1} + db over the population, and whether ESS = (sum w)^2 / sum w^2 >= thr
__device__ __forceinline__ bool smc_ess(SmcShared &sh, const double *F, int i0, int i1, double db, double fmin, double thr,
                                        double &sw, double &sw2) {
    double a = 0.0, b = 0.0;
    for (int i = i0; i < i1; ++i) {
        const double w = smc_weight(F[i], db, fmin);
        a += w;
        b += w * w;
    }
    return block_sums(sh, a, b, thr, sw, sw2);
}

__global__ __launch_bounds__(kSmcThreads) void smc_stage_kernel(const sx_smc_args a, int s) {
    extern __shared__ double F[];  // (P): the values, then the running sums of the weights
    __shared__ SmcShared sh;
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int64_t c = blockIdx.x;
    const int P = (int)a.P;
    const int K = (P + kSmcThreads - 1) / kSmcThreads;
    const int i0 = tid * K < P ? tid * K : P, i1 = i0 + K < P ? i0 + K : P;
    double *st = a.state + c * kStWords;
    const double status = st[kStStatus], stages = st[kStStages], beta0 = st[kStBeta], logz0 = st[kStLogZ];
    double scale = st[kStScale];
    __syncthreads();  // every thread has read the record before thread 0 writes any of it
    double unused0, unused1;
    if (s >= 2 && stages == (double)(s - 1)) {  // step 6 of stage s - 1, whose mutation has run
        double cnt = 0.0;
        for (int i = i0; i < i1; ++i) cnt += (double)a.nacc[c * P + i];
        double total;
        block_sums(sh, cnt, 1.0, 0.0, total, unused1);
        const double r = total / ((double)P * (double)a.steps);
        scale = scale * exp(r - a.target);
        if (tid == 0) st[kStAccept] = r, st[kStCount] = total;
    }
    if (status != kSmcRunning) return;  // (frozen, or the closing call: the whole workgroup, on one word)

    const double *fsrc = a.f[(s - 1) & 1] + c * P;
    double lo = kHuge, nfinite = 0.0, nneg = 0.0;
    for (int i = i0; i < i1; ++i) {
        const double f = fsrc[i];
        F[i] = f;
        if (f == f && f < kHuge) {
            if (f > -kHuge)
                nfinite += 1.0, lo = fmin(lo, f);
            else
                nneg += 1.0;
        }
    }
    block_sums(sh, nfinite, nneg, 0.0, nfinite, nneg);
    const double fmin_ = block_min(sh, lo);
    if (nfinite == 0.0 || nneg > 0.0) {
        if (tid == 0) st[kStStatus] = -2.0, st[kStLogZ] = -kHuge;
        return;
    }

    // step 1: the next beta
    const double thr = a.ess * (double)P;
    double sw, sw2, beta;
    if (smc_ess(sh, F, i0, i1, 1.0 - beta0, fmin_, thr, sw, sw2)) {
        beta = 1.0;
    } else {
        double blo = beta0, bhi = 1.0;
#pragma unroll 1
        for (int k = 0; k < kSmcHalvings; ++k) {
            const double mid = (blo + bhi) / 2.0;
            if (smc_ess(sh, F, i0, i1, mid - beta0, fmin_, thr, unused0, unused1))
                blo = mid;
            else
                bhi = mid;
        }
        beta = blo > beta0 ? blo : bhi;
    }
    // step 2: the evidence
    const double db = beta - beta0;
    smc_ess(sh, F, i0, i1, db, fmin_, thr, sw, sw2);
    const double logz = logz0 + (log(sw / (double)P) - db * fmin_);
    const double ess = ((sw * sw) / sw2) / (double)P;

    // step 3: the running sums -- thread totals scanned over the wave (v += v[lane - 1], - 2, ... - 32), the waves' totals added
    // in order, then the thread's own terms one by one on top of (waves before + threads before)
    double tot = 0.0;
    for (int i = i0; i < i1; ++i) tot += smc_weight(F[i], db, fmin_);
    double inc = tot;
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
        const double t = __shfl_up(inc, off, kWave);
        if (lane >= off) inc += t;
    }
    double exc = __shfl_up(inc, 1, kWave);
    if (lane == 0) exc = 0.0;
    if (lane == kWave - 1) sh.part[0][wave] = inc;
    __syncthreads();
    double base = 0.0;
    for (int w = 0; w < wave; ++w) base += sh.part[0][w];
    double run = base + exc;
    for (int i = i0; i < i1; ++i) {
        run += smc_weight(F[i], db, fmin_);
        F[i] = run;
    }
    __syncthreads();
    const double total = F[P - 1];
    const U4 w4 = philox4x32_10(0u, (uint32_t)(c * P), (uint32_t)s, kPurposeSampleResample, a.key0, a.key1);
    const double u = u53(w4.x, w4.y);
    for (int i = tid; i < P; i += kSmcThreads) {
        const double target = (((double)i + u) / (double)P) * total;
        int jlo = 0, jhi = P - 1;  // the least j with cum_j >= target, P - 1 when there is none
        while (jlo < jhi) {
            const int mid = (jlo + jhi) >> 1;
            if (F[mid] >= target)
                jhi = mid;
            else
                jlo = mid + 1;
        }
        a.anc[c * P + i] = jlo;
    }
    if (tid == 0) {
        st[kStStatus] = beta == 1.0 ? 0.0 : (s >= a.maxiter ? -1.0 : kSmcRunning);
        st[kStBeta] = beta, st[kStLogZ] = logz, st[kStEss] = ess, st[kStScale] = scale, st[kStStages] = (double)s;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// The gather kernel: workgroup (c, t) moves axes [16 t, 16 t + 16) of population c.  Thread (r, j) takes particles r, r + 16,
// ... of axis 16 t + j: x_i <- x_{anc_i} into the other buffer, summed on the way (0.0 + its terms in that order); the 16
// threads' sums are added in the order of r; the deviations from the mean the same way in a second pass over what the thread
// itself wrote.  Workgroup (c, 0) also moves the values.
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kGatherAxes *kGatherRows) void smc_gather_kernel(const sx_smc_args a, int s) {
    __shared__ double part[kGatherRows][kGatherAxes + 1];
    const int tid = (int)threadIdx.x, j = tid & (kGatherAxes - 1), r = tid / kGatherAxes;
    const int64_t c = blockIdx.x;
    const int n = a.n, e = (int)blockIdx.y * kGatherAxes + j;
    const int64_t P = a.P;
    const double *st = a.state + c * kStWords;
    if (st[kStStages] != (double)s) return;  // (the whole workgroup: this population takes no part in stage s)
    const double *src = a.x[(s - 1) & 1] + c * P * n;
    double *dst = a.x[s & 1] + c * P * n;
    const int32_t *anc = a.anc + c * P;
    const bool in = e < n;
    const auto ancestor = [&](int64_t i) {  // (the stage kernel's, inside [0, P) by its search; held there whatever anc holds)
        const int64_t k = anc[i];
        return k < 0 ? 0 : (k < P ? k : P - 1);
    };
    const auto total = [&](double v) {
        __syncthreads();
        part[r][j] = v;
        __syncthreads();
        double t = 0.0;
        for (int k = 0; k < kGatherRows; ++k) t += part[k][j];
        return t;
    };
    double sum = 0.0;
    if (in)
        for (int64_t i = r; i < P; i += kGatherRows) {
            const double v = src[ancestor(i) * n + e];
            dst[i * n + e] = v;
            sum += v;
        }
    const double mean = total(sum) / (double)P;
    double dev = 0.0;
    if (in)
        for (int64_t i = r; i < P; i += kGatherRows) {
            const double d = dst[i * n + e] - mean;
            dev += d * d;
        }
    const double sd = sqrt(total(dev) / (double)P);
    if (in && r == 0) {
        const double floor_ = 1.0e-8 * (0.5 * (a.upper[e] - a.lower[e]));
        a.step[c * n + e] = st[kStScale] * (sd > floor_ ? sd : floor_);
    }
    if (blockIdx.y == 0) {
        const double *fsrc = a.f[(s - 1) & 1] + c * P;
        double *fdst = a.f[s & 1] + c * P;
        for (int64_t i = tid; i < P; i += kGatherAxes * kGatherRows) fdst[i] = fsrc[ancestor(i)];
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// The mutation kernel: one row group per particle q = c P + i, mcmc_kernel's geometry and LDS row (X[n] | U[gen_row_stride(n)]).
// s = 0 draws and evaluates the particles and starts the populations' records.
// ---------------------------------------------------------------------------------------------------------------------
template <int FUN, int LPR>
__global__ __launch_bounds__(kMaxWavesPerBlock *kWave) void smc_mutate_kernel(const sx_smc_args a, const PlanArg plan, int s) {
    extern __shared__ double lds[];
    const RowIds<LPR> id(a.C * a.P);
    const int n = a.n, l = id.l;
    const int64_t q = id.rowc, c = q / a.P;
    const sx_sample_args v = chain_view(a);
    double *X = lds + (size_t)id.slot * sample_row_doubles(kMcmc, n);
    double *U = X + n;
    if (s == 0) {
        for (int e = l; e < n; e += LPR) U[e] = initial_value<LPR>(v, q, e);
        const double f = row_objective<FUN, LPR, 0, 0>(U, n, plan, l);
        if (id.active) {
            for (int e = l; e < n; e += LPR) a.x[0][q * n + e] = U[e];
            if (l == 0) {
                a.f[0][q] = f;
                if (q == c * a.P) start_record(a, c);
            }
        }
        return;
    }
    const double *st = a.state + c * kStWords;
    const bool live = id.active && st[kStStages] == (double)s;  // (the others run along and store nothing)
    const double beta = st[kStBeta];
    double *xq = a.x[s & 1] + q * n;
    const double *step = a.step + c * n;
    for (int e = l; e < n; e += LPR) X[e] = xq[e];
    ChainState cs;
    cs.start(a.f[s & 1][q]);
    const int M = a.steps;
#pragma unroll 1
    for (int m = 1; m <= M; ++m) {
        const int64_t g = (int64_t)(s - 1) * M + m;
        mcmc_propose<LPR>(
            v, (uint32_t)q, g, X, l, 0, n, [&](int e) { return step[e]; }, [&](int e, double val) { U[e] = val; });
        // (a proposal outside the box is evaluated too and its value dropped: the rows of a wave stay in step)
        const double fU = row_objective<FUN, LPR, 0, 0>(U, n, plan, l);
        const bool feasible = row_in_box<LPR>(v, U, n, l);
        const Decision r = chain_decide(cs, v, (uint32_t)q, g, true, feasible, beta * (cs.fcur - fU), fU);
        if (r.accept)
            for (int e = l; e < n; e += LPR) X[e] = U[e];
    }
    if (live) {
        for (int e = l; e < n; e += LPR) xq[e] = X[e];
        if (l == 0) a.f[s & 1][q] = cs.fcur, a.nacc[q] = cs.nacc;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Around a caller's objective: step m of stage s is propose -> objective -> decide, the particles in device memory; the same
// functions on the same values.  (s, m) = (0, 0): the draw, and the start of the records behind the objective.
// ---------------------------------------------------------------------------------------------------------------------
template <int LPR>
__global__ __launch_bounds__(kMaxWavesPerBlock *kWave) void smc_propose_kernel(const sx_smc_args a, int s, int m,
                                                                               double *__restrict__ prop) {
    const RowIds<LPR> id(a.C * a.P);
    const int n = a.n, l = id.l;
    const int64_t q = id.rowc, c = q / a.P;
    const sx_sample_args v = chain_view(a);
    double *U = prop + q * n;
    if (s == 0) {
        for (int e = l; e < n; e += LPR) {
            const double x = initial_value<LPR>(v, q, e);
            if (id.active) U[e] = x;
        }
        return;
    }
    const double stages = a.state[c * kStWords + kStStages];
    const bool live = stages == (double)s;
    // (an ended population's particles are where its last stage left them, in the buffer its own record names -- not in x[s & 1])
    const double *X = a.x[(live ? s : (int)stages) & 1] + q * n;
    const double *step = a.step + c * n;
    const int64_t g = (int64_t)(s - 1) * a.steps + m;
    mcmc_propose<LPR>(
        v, (uint32_t)q, g, X, l, 0, n, [&](int e) { return step[e]; },
        [&](int e, double val) {  // (a frozen particle proposes itself: the objective is called on points of the box only)
            if (id.active) U[e] = live ? val : X[e];
        });
}

template <int LPR>
__global__ __launch_bounds__(kMaxWavesPerBlock *kWave) void smc_decide_kernel(const sx_smc_args a, int s, int m,
                                                                              const double *__restrict__ prop,
                                                                              const double *__restrict__ fprop) {
    const RowIds<LPR> id(a.C * a.P);
    const int n = a.n, l = id.l;
    const int64_t q = id.rowc, c = q / a.P;
    const sx_sample_args v = chain_view(a);
    const double *U = prop + q * n;
    const double fU = fprop[q];
    if (s == 0) {
        if (id.active) {
            for (int e = l; e < n; e += LPR) a.x[0][q * n + e] = U[e];
            if (l == 0) {
                a.f[0][q] = fU;
                if (q == c * a.P) start_record(a, c);
            }
        }
        return;
    }
    const double *st = a.state + c * kStWords;
    const bool live = id.active && st[kStStages] == (double)s;
    const double beta = st[kStBeta];
    const int64_t g = (int64_t)(s - 1) * a.steps + m;
    ChainState cs;
    cs.start(a.f[s & 1][q]);
    cs.nacc = m == 1 ? 0 : a.nacc[q];
    const bool feasible = row_in_box<LPR>(v, U, n, l);
    const Decision r = chain_decide(cs, v, (uint32_t)q, g, true, feasible, beta * (cs.fcur - fU), fU);
    if (live) {
        double *X = a.x[s & 1] + q * n;
        if (r.accept)
            for (int e = l; e < n; e += LPR) X[e] = U[e];
        if (l == 0) a.f[s & 1][q] = cs.fcur, a.nacc[q] = cs.nacc;
    }
}

// What every entry point `who` requires of its arguments before it launches stage s (`resident`: fun_id names the objective)
int check_smc_args(const char *who, const sx_smc_args *a, int s, int smax, bool resident) {
    SX_SAMPLE_REQUIRE(a != nullptr, "null args");
    SX_SAMPLE_REQUIRE(a->x[0] && a->x[1] && a->f[0] && a->f[1] && a->anc && a->nacc && a->step && a->state, "null state pointer");
    SX_SAMPLE_REQUIRE(a->lower && a->upper, "bounds missing");
    SX_SAMPLE_REQUIRE(a->C >= 1 && a->P >= 4 && a->P <= kSmcMaxParticles && a->C * a->P < (int64_t)1 << 31,
                      "bad shape: C >= 1 populations of 4 <= P <= sx_smc_max_particles() particles, C P < 2^31");
    SX_SAMPLE_REQUIRE(a->n >= 1 && a->n <= kWideFrom, "rows of 1 to sx_wide_from() elements");
    SX_SAMPLE_REQUIRE(!resident || (a->fun_id >= 0 && a->fun_id < SX_FUN_COUNT), "unknown objective");
    SX_SAMPLE_REQUIRE(a->steps >= 1 && a->maxiter >= 1 && (int64_t)a->steps * a->maxiter < (int64_t)1 << 31,
                      "steps >= 1, maxiter >= 1, steps * maxiter < 2^31");
    SX_SAMPLE_REQUIRE(a->ess > 0.0 && a->ess < 1.0, "ess outside (0, 1)");
    SX_SAMPLE_REQUIRE(a->target > 0.0 && a->target < 1.0, "target outside (0, 1)");
    SX_SAMPLE_REQUIRE(a->scale > 0.0 && a->scale < kHuge, "scale is not a finite number > 0");
    SX_SAMPLE_REQUIRE(s >= 0 && s <= smax, "stage outside its range");
    return 0;
}

inline Geometry particle_geometry(const sx_smc_args *a) {  // (the unfused kernels: the row kernels' 16-row cap, no LDS)
    const int waves = waves_per_workgroup(a->n, 0);
    const int rows = waves * (kWave / lanes_per_row(a->n));
    return Geometry{(unsigned)((a->C * a->P + rows - 1) / rows), (unsigned)(waves * kWave), 0};
}

int mutate(const char *who, const sx_smc_args *a, int s, void *stream) {
    PlanArg plan;
    if (make_plan_arg(a->fun_id, a->n, &plan)) return -1;
    void (*kern)(const sx_smc_args, const PlanArg, int) = nullptr;
    SX_DISPATCH_LPR(a->n, SX_DISPATCH_FUN(a->fun_id, (kern = smc_mutate_kernel<FUN, LPR>)))
    const int waves = sample_waves(kMcmc, a->n);
    const int rows = waves * (kWave / lanes_per_row(a->n));
    const size_t lds = (size_t)rows * sample_row_doubles(kMcmc, a->n) * sizeof(double);
    SX_SAMPLE_REQUIRE(lds <= 160 * 1024, "one wave's particles do not fit the 160 KiB of LDS of a workgroup");
    if (lds > 64 * 1024) SX_HIP(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    return Enqueue((hipStream_t)stream)
        .kernel(kern, dim3((unsigned)((a->C * a->P + rows - 1) / rows)), dim3(waves * kWave), lds, *a, plan, s);
}

}  // namespace

extern "C" int sx_smc_args_bytes(void) { return (int)sizeof(sx_smc_args); }
extern "C" int sx_smc_max_particles(void) { return kSmcMaxParticles; }

extern "C" int sx_smc_init(const sx_smc_args *a, void *stream) {
    const char *who = "sx_smc_init";
    if (check_smc_args(who, a, 0, 0, true)) return -1;
    return mutate(who, a, 0, stream);
}

extern "C" int sx_smc_stage(const sx_smc_args *a, int s, void *stream) {
    const char *who = "sx_smc_stage";
    if (check_smc_args(who, a, s, a ? a->maxiter + 1 : 0, false)) return -1;
    SX_SAMPLE_REQUIRE(s >= 1, "stage outside its range");
    const size_t lds = (size_t)a->P * sizeof(double);
    if (lds > 48 * 1024)
        SX_HIP(hipFuncSetAttribute((const void *)smc_stage_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    return Enqueue((hipStream_t)stream).kernel(smc_stage_kernel, dim3((unsigned)a->C), dim3(kSmcThreads), lds, *a, s);
}

extern "C" int sx_smc_resample(const sx_smc_args *a, int s, void *stream) {
    const char *who = "sx_smc_resample";
    if (check_smc_args(who, a, s, a ? a->maxiter : 0, false)) return -1;
    SX_SAMPLE_REQUIRE(s >= 1, "stage outside its range");
    const unsigned tiles = (unsigned)((a->n + kGatherAxes - 1) / kGatherAxes);
    return Enqueue((hipStream_t)stream)
        .kernel(smc_gather_kernel, dim3((unsigned)a->C, tiles), dim3(kGatherAxes * kGatherRows), 0, *a, s);
}

extern "C" int sx_smc_mutate(const sx_smc_args *a, int s, void *stream) {
    const char *who = "sx_smc_mutate";
    if (check_smc_args(who, a, s, a ? a->maxiter : 0, true)) return -1;
    SX_SAMPLE_REQUIRE(s >= 1, "stage outside its range");
    return mutate(who, a, s, stream);
}

extern "C" int sx_smc_propose(const sx_smc_args *a, int s, int m, double *prop, void *stream) {
    const char *who = "sx_smc_propose";
    if (check_smc_args(who, a, s, a ? a->maxiter : 0, false)) return -1;
    SX_SAMPLE_REQUIRE(prop != nullptr, "null proposal array");
    SX_SAMPLE_REQUIRE(s == 0 ? m == 0 : (m >= 1 && m <= a->steps), "step outside [1, steps] (stage 0: step 0)");
    const Geometry g = particle_geometry(a);
    Enqueue q((hipStream_t)stream);
    SX_DISPATCH_LPR(a->n, return q.kernel(smc_propose_kernel<LPR>, dim3(g.blocks), dim3(g.threads), 0, *a, s, m, prop))
    return -1;
}

extern "C" int sx_smc_decide(const sx_smc_args *a, int s, int m, const double *prop, const double *fprop, void *stream) {
    const char *who = "sx_smc_decide";
    if (check_smc_args(who, a, s, a ? a->maxiter : 0, false)) return -1;
    SX_SAMPLE_REQUIRE(prop && fprop, "null proposal / value array");
    SX_SAMPLE_REQUIRE(s == 0 ? m == 0 : (m >= 1 && m <= a->steps), "step outside [1, steps] (stage 0: step 0)");
    const Geometry g = particle_geometry(a);
    Enqueue q((hipStream_t)stream);
    SX_DISPATCH_LPR(a->n, return q.kernel(smc_decide_kernel<LPR>, dim3(g.blocks), dim3(g.threads), 0, *a, s, m, prop, fprop))
    return -1;
}
