// Many independent DE runs in one launch: one workgroup per run, resident from the initial population to the run's own
// termination (include/stochopy_hip.h, sx_de_runs_args).  A small population (the reference's default is popsize = 10) fills one
// or two workgroups of the generation kernels and pays a launch per generation; R such runs under R seeds fill the device
// instead, and a generation costs two workgroup barriers.
//
// Reference code replaced (paths relative to the reference checkout), R times over:
//   stochopy/optimize/de/_de.py:176-301       de: initial population and best (:208-218), the generation loop (:236-283)
//   stochopy/optimize/de/_de.py:314-351       de_sync (mutation, crossover); de/_strategy.py:1-46, de/_constraints.py:13-28
//   stochopy/optimize/_common.py:109-120      the Latin hypercube (in-kernel draws: philox_lhs_element)
//   stochopy/optimize/_common.py:123-158      selection_sync + argmin + the termination ladder
//
// LDS of a run (doubles): buf[2][P][gen_row_stride(n)] | fit[P] | 4 words of broadcast.  Generation g lives in buf[g & 1] (as in
// sx_de_args).  A row group builds its trial IN its row's slot of the other buffer -- that slot is the staging area
// row_objective wants (the vector, 8 doubles of padding, the long rows' leaf sums) --, evaluates it there and, if the trial
// does not win, overwrites it with the current row: the slot belongs to the row group, so none of this needs a barrier, and
// everything a generation READS (own row, donors, best row) is in the current buffer, which nobody writes (deferred updating).
// Behind the generation's barrier wavefront 0 finds the best of fit[P], the step of the best against the previous best row
// (still resident: the current buffer) and the status; a second barrier publishes them.
//
// Same bits as the single-run kernels (sx_de_kernel.hpp, sx_unfused.hip): the same device functions with the same counters
// -- row = the row within the run, the run's own key --, the same arithmetic (-ffp-contract=off), the same orders of summation.
#include "sx_device.hpp"
#include "sx_host.hpp"
#include "sx_rowops.hpp"
#include "sx_runs.hpp"

namespace sx {
int make_plan_arg(int fun_id, int n, PlanArg *out);
}
using namespace sx;

namespace {

constexpr int kStep = 4;                    // row steps per batch: one pair of Philox calls (de_propose_kernel's layout)
constexpr int kBroadcastWords = 4;          // best value, best row, status, (spare)
constexpr int kFinalThreads = 256;          // threads of select_finalize_kernel (sx_core.hip): its dx sums in their order

inline int64_t runs_lds_doubles(int64_t P, int n) { return 2 * P * gen_row_stride(n) + P + kBroadcastWords; }

// Waves of a run's workgroup.  What a run needs is LDS, so few runs fit a CU when the population is large: those take the
// most waves a workgroup may have (one or two resident workgroups have to fill the CU's four SIMDs on their own).  Small
// populations take four -- more resident runs per CU, whose one-wavefront steps behind the barrier then overlap with other
// runs' generations -- and loop over their rows in passes.  Never more waves than rows to carry.  Results do not depend on it.
inline int runs_waves(int64_t P, int n) {
    const int rpw = kWave / lanes_per_row(n);
    const bool few_fit = runs_lds_doubles(P, n) * (int64_t)sizeof(double) > kLdsLimit / 4;
    const int64_t want = few_fit ? kMaxWavesPerBlock : 4, need = (P + rpw - 1) / rpw;
    return (int)(need < want ? need : want);
}

// minimum wavefronts per SIMD asked of the compiler: 4 caps the kernels at 128 VGPRs.  Rows of up to 128 elements take 88 ... 119
// on their own (Griewank: 136); what the cap costs is a few spilled registers in the whole-wave kernels of Griewank and Quartic,
// whose compile-time plans for long rows take up to 228 uncapped
#ifndef SX_DE_RUNS_WAVES
#define SX_DE_RUNS_WAVES 4
#endif
template <int FUN, int LPR>
__global__ __launch_bounds__(kMaxWavesPerBlock *kWave, SX_DE_RUNS_WAVES) void de_runs_kernel(const sx_de_runs_args a, const PlanArg plan,
                                                                                              const DeSweep sw) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int n = a.n, P = (int)a.P;
    const int S = gen_row_stride(n);
    double *const buf0 = lds, *const buf1 = lds + (size_t)P * S;
    double *const fit = buf1 + (size_t)P * S;
    double *const s_bf = fit + P;                                        // broadcast words, written by wavefront 0
    int *const s_bi = reinterpret_cast<int *>(s_bf + 1), *const s_status = reinterpret_cast<int *>(s_bf + 2);
    const int64_t run = blockIdx.x;
    const RowIds<LPR> id(a.P);  // wave / lane / l / slot only: the rows are this run's, taken in passes of `rpp`
    const int l = id.l, rpp = (int)(blockDim.x >> 6) * RowIds<LPR>::RPW;
    const uint32_t key0 = a.keys[2 * run], key1 = a.keys[2 * run + 1];
    // the run's own settings (uniform in the workgroup): element `run` of a sweep's arrays, else the struct's scalars
    const int strategy = run_setting(sw.strategy, run, a.strategy), k = donors_of(strategy);
    const bool repair = a.constraints != 0;
    const bool use_best = strategy == SX_DE_BEST1BIN || strategy == SX_DE_BEST2BIN;
    const double F = run_setting(sw.F, run, a.F), CR = run_setting(sw.CR, run, a.CR);
    if ((unsigned)strategy > (unsigned)SX_DE_BEST2BIN || k > P - 1) {  // an element the launch could not read: no run
        if (threadIdx.x == 0) {
            a.funs[run] = __builtin_nan("");
            a.nits[run] = 0;
            a.statuses[run] = SX_STATUS_NONE;
        }
        return;
    }

    int it = 0;    // the generation the population holds (the reference's `it`); 0: nothing yet
    int gb = 0;    // its best row
    double bf = 0.0;
    int status = SX_STATUS_NONE;
    const int nq = (n + LPR - 1) / LPR;
    for (;;) {
        // ---- generation it + 1 into buf[(it + 1) & 1].  Generation 1 is the initial population (de/_de.py:208-218); the
        //      others (de/_de.py:314-351 + _common.py:123-130) read the current buffer only
        const double *__restrict__ cur = (it & 1) ? buf1 : buf0;
        double *nxt = (it & 1) ? buf0 : buf1;
        const uint32_t gen = (uint32_t)(it + 1);
        const double *__restrict__ gbrow = cur + (size_t)gb * S;
        for (int row = id.slot; row < P; row += rpp) {
            const uint32_t grow = (uint32_t)row;
            const double *__restrict__ xi = cur + (size_t)row * S;
            double *U = nxt + (size_t)row * S;
            if (it == 0) {
                if (a.x0 != nullptr) {
                    const double *__restrict__ src = a.x0 + run * a.x0_stride + (int64_t)row * n;
                    for (int e = l; e < n; e += LPR) U[e] = src[e];
                } else {
                    for (int e = l; e < n; e += LPR)
                        U[e] = philox_lhs_element((uint64_t)row, e, a.P, n, a.lower[e], a.upper[e], key0, key1);
                }
            } else {
                // de_propose_row (sx_unfused.hpp) onto a resident row, left apart: a correction made there is owed here
                int64_t d[kMaxDonors];
                int irand;
                philox_donors(a.P, k, row, grow, gen, key0, key1, n, d, irand);
                for (int q0 = 0; q0 < nq; q0 += kStep) {
                    double r[kStep];
#pragma unroll
                    for (int t = 0; t < kStep; t += 2) {  // 53-bit crossover uniforms: slot (q >> 1) * LPR + l, two per call
                        const U4 w = philox4x32_10((uint32_t)((q0 + t) >> 1) * (uint32_t)LPR + (uint32_t)l, grow, gen,
                                                   kPurposeDeCross, key0, key1);
                        r[t] = u53(w.x, w.y);
                        r[t + 1] = u53(w.z, w.w);
                    }
#pragma unroll
                    for (int t = 0; t < kStep; ++t) {
                        const int e = (q0 + t) * LPR + l;
                        if (e >= n) continue;
                        double dv[kMaxDonors];
#pragma unroll
                        for (int s = 0; s < kMaxDonors; ++s) dv[s] = s < k ? cur[(size_t)d[s] * S + e] : 0.0;
                        const double g = use_best ? gbrow[e] : 0.0;
                        const double v = de_mutant(strategy, g, dv[0], dv[1], dv[2], dv[3], dv[4], F);
                        double c = (e == irand || r[t] <= CR) ? v : xi[e];  // de/_de.py:341-344
                        if (repair && (c < a.lower[e] || c > a.upper[e]))  // de/_constraints.py:21-26
                            c = a.lower[e] +
                                (a.upper[e] - a.lower[e]) * philox_u53(e, LPR, grow, gen, kPurposeDeResample, key0, key1);
                        U[e] = c;
                    }
                }
            }
            const double fc = row_objective<FUN, LPR>(U, n, plan, l);
            const bool better = it == 0 || fc < fit[row];  // _common.py:127 strict <
            lds_wave_fence();                              // the objective has read the slot
            if (!better) {
                for (int e = l; e < n; e += LPR) U[e] = xi[e];
            } else if (l == 0) {
                fit[row] = fc;
            }
        }
        ++it;

        // ---- best of that generation, step of the best, status (_common.py:131-158): wavefront 0
        __syncthreads();
        if (id.wave == 0) {
            double wf = __builtin_huge_val();
            int64_t wi = INT64_MAX;
            for (int c0 = 0; c0 < P; c0 += kWave) {  // lanes in row order, chunks in row order: np.argmin's first minimum
                const int r = c0 + id.lane;
                double f = r < P ? fit[r] : __builtin_huge_val();
                int64_t i = r < P ? (int64_t)r : INT64_MAX;
                wave_argmin_ordered(f, i);
                argmin_combine(wf, wi, f, i);
            }
            int st = SX_STATUS_NONE;
            if (it >= 2) {  // the reference does not test the initial population
                // dx = ||xbest_prev - x[k]|| (_common.py:135) in select_finalize_kernel's order: thread t of 256 adds the squares
                // of its elements t, t + 256, ... in order, a wavefront's 64 sums meet in an xor butterfly (32 ... 1), the four
                // wavefronts' totals are added in order.  Here one wavefront plays the four in turn.  Both rows are resident:
                // the previous best in the buffer this generation read, the new one in the buffer it wrote.
                const double *__restrict__ prev = gbrow;
                const double *__restrict__ best = nxt + (size_t)wi * S;
                double ss = 0.0;
                for (int w = 0; w < kFinalThreads / kWave; ++w) {
                    double acc = 0.0;
                    for (int e = w * kWave + id.lane; e < n; e += kFinalThreads) {
                        const double d = prev[e] - best[e];
                        acc += d * d;
                    }
#pragma unroll
                    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, kWave);
                    ss += acc;
                }
                const double dx = sqrt(ss);
                // best_step's sum (sx_unfused.hpp) and sync_status (sx_rowops.hpp), left apart: a correction made there is owed here
                if (dx <= a.xtol && wf <= a.ftol)
                    st = 0;
                else if (wf <= a.ftol)
                    st = 1;
                else if (it >= a.maxiter)
                    st = -1;
            }
            if (id.lane == 0) {
                *s_bf = wf;
                *s_bi = (int)wi;
                *s_status = st;
            }
        }
        __syncthreads();
        bf = *s_bf, gb = *s_bi, status = *s_status;
        if (status != SX_STATUS_NONE) break;  // this run is over; the other runs' workgroups know nothing of it
    }

    // ---- the run's results
    const double *__restrict__ fin = (it & 1) ? buf1 : buf0;
    for (int e = (int)threadIdx.x; e < n; e += (int)blockDim.x) a.xs[run * n + e] = fin[(size_t)gb * S + e];
    if (a.xfinal != nullptr) {
        double *__restrict__ out = a.xfinal + run * a.P * n;
        for (int row = id.slot; row < P; row += rpp)
            for (int e = l; e < n; e += LPR) out[(int64_t)row * n + e] = fin[(size_t)row * S + e];
    }
    if (threadIdx.x == 0) {
        a.funs[run] = bf;
        a.nits[run] = it;
        a.statuses[run] = status;
    }
}

}  // namespace

extern "C" int64_t sx_de_runs_lds_bytes(int64_t P, int n) {
    if (P < 2 || P > kLdsLimit || n < 1 || n > kWideFrom) return -1;
    const int64_t bytes = runs_lds_doubles(P, n) * (int64_t)sizeof(double);
    return bytes <= kLdsLimit ? bytes : -1;
}

extern "C" int sx_de_runs_sweep_launch(const sx_de_runs_args *a, const double *F, const double *CR, const int32_t *strategy,
                                       void *stream) {
    SX_REQUIRE(a != nullptr, "sx_de_runs_launch: null args");
    SX_REQUIRE(a->keys && a->lower && a->upper && a->xs && a->funs && a->nits && a->statuses,
               "sx_de_runs_launch: null device pointer");
    SX_REQUIRE(a->R >= 1 && a->R < (int64_t)1 << 31 && a->P >= 2 && a->n >= 1 && a->n <= kWideFrom,
               "sx_de_runs_launch: bad shape");
    SX_REQUIRE(a->fun_id >= 0 && a->fun_id < SX_FUN_COUNT, "sx_de_runs_launch: unknown objective");
    SX_REQUIRE(a->strategy >= 0 && a->strategy <= SX_DE_BEST2BIN, "sx_de_runs_launch: unknown strategy");
    SX_REQUIRE(a->P - 1 >= donors_of(a->strategy), "sx_de_runs_launch: population too small for the strategy");
    SX_REQUIRE(a->x0 == nullptr || a->x0_stride == 0 || a->x0_stride == a->P * a->n, "sx_de_runs_launch: bad x0 stride");
    const int64_t lds = sx_de_runs_lds_bytes(a->P, a->n);
    SX_REQUIRE(lds > 0, "sx_de_runs_launch: the run's two populations do not fit one workgroup's LDS");
    PlanArg plan;
    if (make_plan_arg(a->fun_id, a->n, &plan)) return -1;
    const int threads = runs_waves(a->P, a->n) * kWave;
    const DeSweep sweep = {F, CR, strategy};
    SX_DISPATCH_LPR(a->n, SX_DISPATCH_FUN(a->fun_id, return enqueue_runs(de_runs_kernel<FUN, LPR>, *a, plan, sweep, threads, lds, stream)))
    return -1;
}

extern "C" int sx_de_runs_launch(const sx_de_runs_args *a, void *stream) {
    return sx_de_runs_sweep_launch(a, nullptr, nullptr, nullptr, stream);
}
