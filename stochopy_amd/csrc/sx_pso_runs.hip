// Many independent PSO / CPSO runs in one launch: one workgroup per run, resident from the initial swarm to the run's own
// termination (include/stochopy_hip.h, sx_pso_runs_args).  A swarm of 10 ... 64 particles fills one or two workgroups of the
// generation kernel and pays two (PSO) to five (CPSO) launches per generation; R such runs under R seeds fill the device
// instead, and a generation costs two workgroup barriers (CPSO: one more for the radius, one more when rows restart).
//
// Reference code replaced (paths relative to the reference checkout), R times over:
//   stochopy/optimize/cpso/_cpso.py:182-321   cpso: initial swarm (:215-247), the generation loop (:257-307)
//   stochopy/optimize/cpso/_cpso.py:324-361   mutation (left to right) and pso_sync
//   stochopy/optimize/cpso/_constraints.py:4-10, 44-53  NoConstraint / Shrink (sync form)
//   stochopy/optimize/cpso/_cpso.py:405-426   restart (radius, nw, worst-nw reset)
//   stochopy/optimize/_common.py:109-120      the Latin hypercube (in-kernel draws: philox_lhs_element)
//   stochopy/optimize/_common.py:123-158      selection_sync + argmin + the termination ladder
//
// LDS of a run (doubles):
//   X[P][gen_row_stride(n)] | V[P][n] | pbest[P][n] | pbestfit[P] | gbest[n] | rad[P] | 4 words of broadcast
// when that is within the 160 KiB a workgroup may declare; a larger swarm keeps everything but V there,
//   X[P][gen_row_stride(n)] | pbest[P][n] | pbestfit[P] | gbest[n] | rad[P] | 4 words of broadcast
// and its velocities in the run's (P, n) slice of the caller's workspace (sx_pso_runs_args.vwork, sx_pso_runs_workspace_bytes).
// V is the array that can leave: an element of V is only ever read and written by the one lane that owns it (lane e % LPR of
// the row's group, the same thread in every generation, in the restart too), so it needs no fence, no barrier and no
// coherence beyond a thread's own program order, wherever it lives; X is the objective's staging area and pbest is read by
// wavefront 0.  Same arithmetic, same bits.
// A row's slot of X is the staging area row_objective wants (the vector, 8 doubles of padding, the long rows' leaf sums): the
// new position is built and evaluated in place there.  V and pbest are read and written element by element by the lanes that
// own the elements and need no padding: they are packed, n doubles a row.
//
// A row group owns its rows of X, V, pbest and its pbestfit entries; besides those a generation reads the gbest row only, which
// nobody writes during a generation: no barrier inside one.  (Shrink's raw velocity waits in the row's own V slot for the
// row-wide beta.)  Behind the generation's barrier wavefront 0 finds the best of pbestfit[P], the step of the best against
// gbest, the status, and then COPIES pbest[best] into gbest -- the next generation may overwrite that pbest row while other
// rows still read gbest --; a second barrier publishes best value and status.
// CPSO, when the run goes on: every row leaves its distance to the new gbest in rad[row]; barrier; every wavefront takes the
// maximum of rad[P] (the same value in all of them) and, if the swarm has contracted, the number nw of rows to restart.  Row r
// restarts when fewer than nw rows have a pbestfit key above its own (= its key is at least the nw-th largest: the device
// rule of pso_restart_select_kernel, ties at the threshold all restart).  The row groups first count, over the still
// unchanged pbestfit[P], for all their rows (a bit per pass); barrier; then re-seed their own rows.  Nothing else is needed
// before the next generation: the re-seeded state is the row's own.
//
// Same bits as the single-run kernels (sx_pso.hip, sx_core.hip select_finalize_kernel): the same device functions with the
// same counters -- row = the row within the run, the run's own key --, the same arithmetic (-ffp-contract=off), the same orders
// of summation.
#include "sx_device.hpp"
#include "sx_host.hpp"
#include "sx_rowops.hpp"
#include "sx_runs.hpp"

namespace sx {
int make_plan_arg(int fun_id, int n, PlanArg *out);
}
using namespace sx;

namespace {

constexpr int kStep = 2;                   // row steps per Philox call: two 53-bit uniforms
constexpr int kBroadcastWords = 4;         // best value, status, (two spare: gbest is a copy, nobody needs the best row)
constexpr int kMaxPasses = 64;             // passes over the rows: the restart flags of a row group are one 64-bit word

// V in LDS when the whole swarm fits, else in the caller's workspace (see the header comment)
inline int64_t runs_lds_doubles(int64_t P, int n, bool v_in_lds) {
    return P * ((int64_t)gen_row_stride(n) + (v_in_lds ? 2 : 1) * (int64_t)n + 2) + n + kBroadcastWords;
}
inline bool runs_v_in_lds(int64_t P, int n) { return runs_lds_doubles(P, n, true) * (int64_t)sizeof(double) <= kLdsLimit; }
inline int64_t runs_lds_doubles(int64_t P, int n) { return runs_lds_doubles(P, n, runs_v_in_lds(P, n)); }

// Waves of a run's workgroup: sx_de_runs.hip's rule.  Few runs fit a CU when the swarm is large: those take the most waves a
// workgroup may have; small swarms take four and loop over their rows in passes.  Never more waves than rows to carry.
// Results do not depend on it.
inline int runs_waves(int64_t P, int n) {
    const int rpw = kWave / lanes_per_row(n);
    const bool few_fit = runs_lds_doubles(P, n) * (int64_t)sizeof(double) > kLdsLimit / 4;
    const int64_t want = few_fit ? kMaxWavesPerBlock : 4, need = (P + rpw - 1) / rpw;
    return (int)(need < want ? need : want);
}

constexpr int kRunsFinalThreads = 256;  // threads of select_finalize_kernel (sx_core.hip): its dx sums in their order

// The one-wavefront step behind a generation: the best of the run's fitness values, the step of the best and the status
// (_common.py:131-158), in the single-run kernels' own orders.  sx_de_runs.hip holds the same statements inline: as a function
// shared by both kernels they cost de_runs_kernel 1 ... 3 VGPRs in every instantiation and 2 ... 6 more spilled registers in the
// five that spill, so there are two copies.
// Called by all 64 lanes of ONE wavefront, behind the generation's barrier.  fit[P]: the values to take the arg-min of (lanes
// in row order, chunks in row order: np.argmin's first minimum) -> wf, wi in every lane.  `it` is the generation just finished;
// from the second on (the reference does not test the initial one) the status comes from
//   dx = ||prev - rows[wi]|| (_common.py:135) in select_finalize_kernel's order: thread t of 256 adds the squares of its elements
//   t, t + 256, ... in order, a wavefront's 64 sums meet in an xor butterfly (32 ... 1), the four wavefronts' totals are added
//   in order.  Here one wavefront plays the four in turn.
// Returns the status (SX_STATUS_NONE: the run goes on).  Writes nothing.
__device__ __forceinline__ int runs_best_status(const double *fit, const int P, const double *__restrict__ prev,
                                                const double *rows, const int stride, const int n, const int it,
                                                const int maxiter, const double xtol, const double ftol, const int lane,
                                                double &wf, int64_t &wi) {
    wf = __builtin_huge_val();
    wi = INT64_MAX;
    for (int c0 = 0; c0 < P; c0 += kWave) {
        const int r = c0 + lane;
        double f = r < P ? fit[r] : __builtin_huge_val();
        int64_t i = r < P ? (int64_t)r : INT64_MAX;
        wave_argmin_ordered(f, i);
        argmin_combine(wf, wi, f, i);
    }
    int st = SX_STATUS_NONE;
    if (it >= 2) {
        const double *__restrict__ best = rows + (size_t)wi * stride;
        double ss = 0.0;
        for (int w = 0; w < kRunsFinalThreads / kWave; ++w) {
            double acc = 0.0;
            for (int e = w * kWave + lane; e < n; e += kRunsFinalThreads) {
                const double d = prev[e] - best[e];
                acc += d * d;
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, kWave);
            ss += acc;
        }
        const double dx = sqrt(ss);
        // best_step's sum (sx_unfused.hpp) and sync_status (sx_rowops.hpp), left apart: a correction made there is owed here
        if (dx <= xtol && wf <= ftol)
            st = 0;
        else if (wf <= ftol)
            st = 1;
        else if (it >= maxiter)
            st = -1;
    }
    return st;
}

// minimum wavefronts per SIMD asked of the compiler: 4 caps the kernels at 128 VGPRs, as in de_runs_kernel
#ifndef SX_PSO_RUNS_WAVES
#define SX_PSO_RUNS_WAVES 4
#endif
template <int FUN, int LPR>
__global__ __launch_bounds__(kMaxWavesPerBlock *kWave, SX_PSO_RUNS_WAVES) void pso_runs_kernel(const sx_pso_runs_args a,
                                                                                               const PlanArg plan,
                                                                                               const PsoSweep sw) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int64_t run = blockIdx.x;
    const int n = a.n, P = (int)a.P;
    const int S = gen_row_stride(n);
    double *const X = lds;
    const bool vlds = a.vwork == nullptr;  // (uniform) V beside X, or in the run's slice of the workspace
    double *const V = X + (size_t)P * S;
    double *const pbest = V + (vlds ? (size_t)P * n : 0);
    double *const Vw = vlds ? nullptr : a.vwork + (size_t)run * P * n;
    double *const pbestfit = pbest + (size_t)P * n;
    double *const gbest = pbestfit + P;
    double *const rad = gbest + n;
    double *const s_bf = rad + P;  // broadcast words, written by wavefront 0
    int *const s_status = reinterpret_cast<int *>(s_bf + 1);
    const RowIds<LPR> id(a.P);  // wave / lane / l / slot only: the rows are this run's, taken in passes of `rpp`
    const int l = id.l, rpp = (int)(blockDim.x >> 6) * RowIds<LPR>::RPW;
    const uint32_t key0 = a.keys[2 * run], key1 = a.keys[2 * run + 1];
    const bool shrink = a.constraints != 0;
    // the run's own settings (uniform in the workgroup): element `run` of a sweep's arrays, else the struct's scalars
    const double w = run_setting(sw.w, run, a.w), c1 = run_setting(sw.c1, run, a.c1), c2 = run_setting(sw.c2, run, a.c2);
    const double gamma = run_setting(sw.gamma, run, a.gamma);

    int it = 0;  // the generation the swarm holds (the reference's `it`); 0: nothing yet
    double bf = 0.0;
    int status = SX_STATUS_NONE;
    const int nq = (n + LPR - 1) / LPR;
    for (;;) {
        // ---- generation it + 1.  Generation 1 is the initial swarm (cpso/_cpso.py:215-247); the others move every particle
        //      (:324-361) against the gbest row, which nobody writes meanwhile
        const uint32_t gen = (uint32_t)(it + 1);
        for (int row = id.slot; row < P; row += rpp) {
            const uint32_t grow = (uint32_t)row;
            double *xr = X + (size_t)row * S;
            double *const vl = V + (size_t)row * n, *const vg = Vw + (size_t)row * n;  // (one of them is used)
            auto vload = [&](int e) -> double { return vlds ? vl[e] : vg[e]; };
            auto vstore = [&](int e, double v) {
                if (vlds)
                    vl[e] = v;
                else
                    vg[e] = v;
            };
            double *pb = pbest + (size_t)row * n;
            if (it == 0) {
                if (a.x0 != nullptr) {
                    const double *__restrict__ src = a.x0 + run * a.x0_stride + (int64_t)row * n;
                    for (int e = l; e < n; e += LPR) xr[e] = src[e];
                } else {
                    for (int e = l; e < n; e += LPR)
                        xr[e] = philox_lhs_element((uint64_t)row, e, a.P, n, a.lower[e], a.upper[e], key0, key1);
                }
                for (int e = l; e < n; e += LPR) {
                    vstore(e, 0.0);
                    pb[e] = xr[e];
                }
            } else {
                // V = w*V + c1*r1*(pbest - X) + c2*r2*(gbest - X) (cpso/_cpso.py:326).  Without Shrink the new position
                // follows at once; with Shrink the raw velocity waits in V for the row-wide beta
                // pso_move_row (sx_unfused.hpp) on resident rows, left apart: a correction made there is owed here
                double beta = __builtin_huge_val();
                for (int q0 = 0; q0 < nq; q0 += kStep) {  // a pair of row steps: one Philox call per purpose
                    // 53-bit r1 and r2: slot (q >> 1) * LPR + l, two per call (pso_generation_kernel's layout)
                    const uint32_t slot = (uint32_t)(q0 >> 1) * (uint32_t)LPR + (uint32_t)l;
                    const U4 wa = philox4x32_10(slot, grow, gen, kPurposePsoR1, key0, key1);
                    const U4 wb = philox4x32_10(slot, grow, gen, kPurposePsoR2, key0, key1);
                    const double r1[kStep] = {u53(wa.x, wa.y), u53(wa.z, wa.w)};
                    const double r2[kStep] = {u53(wb.x, wb.y), u53(wb.z, wb.w)};
#pragma unroll
                    for (int t = 0; t < kStep; ++t) {
                        const int e = (q0 + t) * LPR + l;
                        if (e >= n) continue;
                        const double x = xr[e];
                        const double vn = pso_velocity(w, vload(e), c1, r1[t], pb[e], x, c2, r2[t], gbest[e]);
                        vstore(e, vn);
                        if (shrink) {  // cpso/_constraints.py:22-50: beta = min over violated dims of (bound - x)/v
                            const double xc = x + vn;
                            const double lo = a.lower[e], hi = a.upper[e];
                            if (xc < lo) beta = fmin(beta, (lo - x) / vn);
                            if (xc > hi) beta = fmin(beta, (hi - x) / vn);
                        } else {  // cpso/_constraints.py:4-10: X + V
                            xr[e] = x + vn;
                        }
                    }
                }
                if (shrink) {
                    beta = row_min<LPR>(beta);
                    if (beta == __builtin_huge_val()) beta = 1.0;
                    lds_wave_fence();
                    for (int e = l; e < n; e += LPR) {
                        const double vn = vload(e) * beta;  // V *= beta[:, None]
                        vstore(e, vn);
                        xr[e] = xr[e] + vn;
                    }
                }
            }
            const double fc = row_objective<FUN, LPR>(xr, n, plan, l);
            const bool better = it == 0 || fc < pbestfit[row];  // _common.py:127 strict <
            lds_wave_fence();                                   // every lane of the row has read pbestfit[row]
            if (better) {
                if (it != 0)
                    for (int e = l; e < n; e += LPR) pb[e] = xr[e];
                if (l == 0) pbestfit[row] = fc;
            }
        }
        ++it;

        // ---- best of that generation, step of the best, status (_common.py:131-158), then gbest = pbest[best]: wavefront 0
        __syncthreads();
        if (id.wave == 0) {
            double wf;
            int64_t wi;
            const int st = runs_best_status(pbestfit, P, gbest, pbest, n, n, it, a.maxiter, a.xtol, a.ftol, id.lane, wf, wi);
            lds_wave_fence();  // the step of the best has read gbest
            const double *best = pbest + (size_t)wi * n;
            for (int e = id.lane; e < n; e += kWave) gbest[e] = best[e];
            if (id.lane == 0) {
                *s_bf = wf;
                *s_status = st;
            }
        }
        __syncthreads();
        bf = *s_bf, status = *s_status;
        if (status != SX_STATUS_NONE) break;  // this run is over; the other runs' workgroups know nothing of it

        // ---- competitive restart (cpso/_cpso.py:405-426), for a run that goes on.  It follows a move (:296-300 is inside the
        //      generation loop): the initial swarm is not looked at
        if (gamma != 0.0 && it >= 2) {  // (uniform)
            for (int row = id.slot; row < P; row += rpp) {
                // ||X_row - gbest||: the lane adds its elements l, l + LPR, ... in order, as pso_radius_kernel does
                const double *xr = X + (size_t)row * S;
                double acc = 0.0;
                for (int e = l; e < n; e += LPR) {
                    const double d = xr[e] - gbest[e];
                    acc += d * d;
                }
                acc = sqrt(row_sum<LPR>(acc));
                if (l == 0) rad[row] = acc;
            }
            __syncthreads();
            double m = 0.0;
            for (int r = id.lane; r < P; r += kWave) m = max_nan(m, rad[r]);
            m = wave_max_f64(m);
            const double radius = m / sqrt(4.0 * (double)n);
            int64_t nw = 0;
            if (radius < a.delta) {
                const double inorm = (double)it / (double)a.maxiter;
                nw = (int64_t)(((double)P - 1.0) / (1.0 + exp(1.0 / 0.09 * (inorm - gamma + 0.5))));
            }
            if (nw > 0) {  // (uniform: every wavefront holds the same radius)
                unsigned long long mine = 0ull;  // bit k: the row of pass k restarts
                int k = 0;
                for (int row = id.slot; row < P; row += rpp, ++k) {
                    const unsigned long long key = sort_key(pbestfit[row]);
                    int above = 0;
                    for (int j = l; j < P; j += LPR) above += sort_key(pbestfit[j]) > key ? 1 : 0;
#pragma unroll
                    for (int off = 1; off < LPR; off <<= 1) above += __shfl_xor(above, off, kWave);
                    if ((int64_t)above < nw) mine |= 1ull << k;
                }
                __syncthreads();  // everybody has counted: pbestfit may change
                const uint32_t rgen = (uint32_t)it;  // the generation that just finished (pso_restart_apply_kernel)
                k = 0;
                for (int row = id.slot; row < P; row += rpp, ++k) {
                    if (!((mine >> k) & 1ull)) continue;
                    double *xr = X + (size_t)row * S;
                    double *const vr = vlds ? V + (size_t)row * n : Vw + (size_t)row * n;
                    double *pb = pbest + (size_t)row * n;
                    for (int e = l; e < n; e += LPR) {
                        const double x = a.lower[e] + (a.upper[e] - a.lower[e]) *
                                                          philox_u53(e, LPR, (uint32_t)row, rgen, kPurposePsoRestart, key0, key1);
                        vr[e] = 0.0;
                        xr[e] = x;
                        pb[e] = x;
                    }
                    if (l == 0) pbestfit[row] = 1.0e30;
                }
            }
        }
    }

    // ---- the run's results
    for (int e = (int)threadIdx.x; e < n; e += (int)blockDim.x) a.xs[run * n + e] = gbest[e];
    for (int row = id.slot; row < P; row += rpp) {
        const int64_t base = (run * a.P + row) * n;
        if (a.xfinal != nullptr)
            for (int e = l; e < n; e += LPR) a.xfinal[base + e] = X[(size_t)row * S + e];
        if (a.pbest_final != nullptr)
            for (int e = l; e < n; e += LPR) a.pbest_final[base + e] = pbest[(size_t)row * n + e];
        if (a.pbestfit_final != nullptr && l == 0) a.pbestfit_final[run * a.P + row] = pbestfit[row];
    }
    if (threadIdx.x == 0) {
        a.funs[run] = bf;
        a.nits[run] = it;
        a.statuses[run] = status;
    }
}

}  // namespace

extern "C" int64_t sx_pso_runs_lds_bytes(int64_t P, int n) {
    if (P < 2 || P > kLdsLimit || n < 1 || n > kWideFrom) return -1;
    const int64_t bytes = runs_lds_doubles(P, n) * (int64_t)sizeof(double);
    return bytes <= kLdsLimit ? bytes : -1;
}

extern "C" int64_t sx_pso_runs_workspace_bytes(int64_t R, int64_t P, int n) {
    if (R < 1 || sx_pso_runs_lds_bytes(P, n) < 0) return -1;
    return runs_v_in_lds(P, n) ? 0 : R * P * (int64_t)n * (int64_t)sizeof(double);
}

extern "C" int sx_pso_runs_sweep_launch(const sx_pso_runs_args *a, const double *w, const double *c1, const double *c2,
                                        const double *gamma, void *stream) {
    SX_REQUIRE(a != nullptr, "sx_pso_runs_launch: null args");
    SX_REQUIRE(a->keys && a->lower && a->upper && a->xs && a->funs && a->nits && a->statuses,
               "sx_pso_runs_launch: null device pointer");
    SX_REQUIRE(a->R >= 1 && a->R < (int64_t)1 << 31 && a->P >= 2 && a->n >= 1 && a->n <= kWideFrom,
               "sx_pso_runs_launch: bad shape");
    SX_REQUIRE(a->fun_id >= 0 && a->fun_id < SX_FUN_COUNT, "sx_pso_runs_launch: unknown objective");
    SX_REQUIRE(a->constraints == 0 || a->constraints == 1, "sx_pso_runs_launch: unknown constraints");
    SX_REQUIRE(a->gamma >= 0.0 && a->gamma <= 2.0, "sx_pso_runs_launch: competitivity outside [0, 2]");
    SX_REQUIRE(a->x0 == nullptr || a->x0_stride == 0 || a->x0_stride == a->P * a->n, "sx_pso_runs_launch: bad x0 stride");
    const int64_t lds = sx_pso_runs_lds_bytes(a->P, a->n);
    SX_REQUIRE(lds > 0, "sx_pso_runs_launch: the run's swarm does not fit one workgroup's LDS");
    SX_REQUIRE(runs_v_in_lds(a->P, a->n) || a->vwork != nullptr, "sx_pso_runs_launch: this swarm needs the velocity workspace");
    sx_pso_runs_args args = *a;
    if (runs_v_in_lds(a->P, a->n)) args.vwork = nullptr;  // (the kernel tells the two layouts apart by this pointer)
    const int waves = runs_waves(a->P, a->n);
    const int64_t rpp = (int64_t)waves * (kWave / lanes_per_row(a->n));
    SX_REQUIRE((a->P + rpp - 1) / rpp <= kMaxPasses, "sx_pso_runs_launch: more passes over the rows than restart flags");
    PlanArg plan;
    if (make_plan_arg(a->fun_id, a->n, &plan)) return -1;
    const PsoSweep sweep = {w, c1, c2, gamma};
    SX_DISPATCH_LPR(a->n, SX_DISPATCH_FUN(a->fun_id, return enqueue_runs(pso_runs_kernel<FUN, LPR>, args, plan, sweep,
                                                                         waves * kWave, lds, stream)))
    return -1;
}

extern "C" int sx_pso_runs_launch(const sx_pso_runs_args *a, void *stream) {
    return sx_pso_runs_sweep_launch(a, nullptr, nullptr, nullptr, nullptr, stream);
}
