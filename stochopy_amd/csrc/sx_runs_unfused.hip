// Many independent DE / PSO runs around a CALLER-SUPPLIED ROW-WISE objective: the batched counterpart of sx_unfused.hip
// (include/stochopy_hip.h, sx_runs_rowwise_args).  The objective cannot be fused, so the R populations live in device memory
// -- three (R, P, n) arrays -- and a generation of ALL runs is
//   propose / move kernel  ->  the caller's objective, ONCE, on the stacked (R*P, n) rows  ->  selection kernel  ->
//   one best / termination workgroup per run
// with the same draws, arithmetic and record layout as the single-run kernels: given the same objective values run r is the
// single run of keys[r], bit for bit.
//
// Reference code replaced (paths relative to the reference checkout), R times over:
//   stochopy/optimize/_common.py:109-120      the Latin hypercube (in-kernel draws: philox_lhs_element)
//   stochopy/optimize/de/_de.py:208-218       initial population and best
//   stochopy/optimize/de/_de.py:314-351       de_sync up to the candidates U (mutation, crossover, Random)
//   stochopy/optimize/cpso/_cpso.py:219-247   initial swarm (V = 0, pbest = X) and best
//   stochopy/optimize/cpso/_cpso.py:324-329   mutation (velocity / position) + cpso/_constraints.py:4-53
//   stochopy/optimize/_common.py:123-130      selection_sync after `candfun = fun(cand)`: strict <, in place
//   stochopy/optimize/_common.py:131-158      argmin + the termination ladder
//
// Geometry: every kernel but the last two uses the row geometry of the single-run kernels (lanes_per_row, rows_per_block,
// RowIds), and a workgroup never spans two runs: a run takes per_run = ceil(P / rows_per_block(n)) workgroups, workgroup b
// serves run b / per_run, and its rows are numbered WITHIN the run (RowIds' first_block).  That keeps everything a
// workgroup shares uniform -- the run's state word (a run that has ended returns at entry, whole workgroups at a time), its
// key and settings, its best row -- and makes a run's (part_f, part_i) records the single run's, so the one-workgroup step
// behind the selection reduces the same records in the same order.  What it costs is the ragged last workgroup of every
// run instead of one for the whole batch.  Row addresses are formed in 64 bits (R*P*n may pass 2^31).
#include "sx_device.hpp"
#include "sx_enqueue.hpp"
#include "sx_host.hpp"
#include "sx_rowops.hpp"
#include "sx_runs.hpp"

using namespace sx;

namespace {

constexpr int kStep = 4;  // row steps per batch of the DE kernel (de_propose_kernel's layout)
constexpr int kDe = 0, kPso = 1;

// ---- 1. the initial populations (generation 1).  DE: buffer 1 -- generation g lives in buffer g & 1 -- and cand, the rows
//      the objective is handed, so that it never sees memory nobody wrote; PSO: X, V = 0, pbest = X
template <int LPR>
__global__ __launch_bounds__(kMaxWavesPerBlock *kWave) void runs_init_kernel(const sx_runs_rowwise_args a, const int per_run) {
    const int64_t run = (int64_t)blockIdx.x / per_run;
    const RowIds<LPR> id(a.P, (int)(run * per_run));
    if (!id.active) return;
    const int n = a.n;
    const int64_t at = (run * a.P + id.row) * (int64_t)n;
    const double *__restrict__ src = a.x0 != nullptr ? a.x0 + run * a.x0_stride + id.row * (int64_t)n : nullptr;
    const uint32_t key0 = a.keys[2 * run], key1 = a.keys[2 * run + 1];
    for (int e = id.l; e < n; e += LPR) {
        const double x = src != nullptr
                             ? src[e]
                             : philox_lhs_element((uint64_t)id.row, e, a.P, n, a.lower[e], a.upper[e], key0, key1);
        if (a.method == kDe) {
            a.pop1[at + e] = x;
        } else {
            a.pop0[at + e] = x;
            a.pop1[at + e] = 0.0;
        }
        a.pop2[at + e] = x;
    }
}

// ---- 2. after the objective has evaluated the initial rows: one workgroup per run.  The first-minimum argmin of the run's P
//      values (sx_argmin's rules: argmin_combine / block_argmin), its state, its best row
__global__ __launch_bounds__(kFinalWorkgroup) void runs_start_kernel(const sx_runs_rowwise_args a,
                                                                     const int32_t *__restrict__ strategy) {
    __shared__ double sf[kFinalWorkgroup / kWave];
    __shared__ int64_t si[kFinalWorkgroup / kWave];
    const int64_t run = blockIdx.x, P = a.P;
    const int n = a.n;
    const double *__restrict__ f = a.f + run * P;
    double *__restrict__ fit = a.fit + run * P, *__restrict__ candfit = a.candfit + run * P;
    double bf = __builtin_huge_val();
    int64_t bi = INT64_MAX;
    for (int64_t k = threadIdx.x; k < P; k += kFinalWorkgroup) {
        const double v = f[k];
        fit[k] = v;
        candfit[k] = v;
        argmin_combine(bf, bi, v, k);
    }
    block_argmin(bf, bi, sf, si);
    const double *__restrict__ best = (a.method == kDe ? a.pop1 : a.pop0) + (run * P + bi) * (int64_t)n;
    for (int e = threadIdx.x; e < n; e += kFinalWorkgroup) a.gbest[run * n + e] = best[e];
    if (threadIdx.x == 0) {
        // an element the launch could not read: no run (sx_de_runs_sweep_launch)
        const int s = a.method == kDe ? run_setting(strategy, run, a.strategy) : (int)SX_DE_RAND1BIN;
        const bool none = a.method == kDe && ((unsigned)s > (unsigned)SX_DE_BEST2BIN || (int64_t)donors_of(s) > P - 1);
        sx_state st = {};
        st.it = 1;
        st.gbidx = bi;
        st.gfit = bf;
        st.dx = 0.0;
        st.status = SX_STATUS_NONE;
        st.done = none ? 1 : 0;
        a.state[run] = st;
        if (none) {
            a.funs[run] = __builtin_nan("");
            a.nits[run] = 0;
            a.statuses[run] = SX_STATUS_NONE;
            atomicAdd(a.ended, 1);
        }
    }
}

// ---- 3. DE: candidates of one generation -> cand, per run (de_propose_kernel's in-kernel-draw branch: same statements)
template <int LPR>
__global__ __launch_bounds__(kMaxWavesPerBlock *kWave) void runs_de_propose_kernel(const sx_runs_rowwise_args a, const DeSweep sw,
                                                                                   const int per_run) {
    const int64_t run = (int64_t)blockIdx.x / per_run;
    const sx_state *st = a.state + run;
    if (st->done) return;
    const int n = a.n;
    const int64_t P = a.P, ld = n;
    const RowIds<LPR> id(P, (int)(run * per_run));
    if (!id.active) return;
    const int l = id.l;
    const int64_t row = id.row, it = st->it, base = run * P * ld;
    const uint32_t gen = (uint32_t)(it + 1), grow = (uint32_t)row;
    const uint32_t key0 = a.keys[2 * run], key1 = a.keys[2 * run + 1];
    const double *__restrict__ cur = ((it & 1) ? a.pop1 : a.pop0) + base;
    const double *__restrict__ xi = cur + row * ld;
    // the run's own settings (uniform in the workgroup): element `run` of a sweep's arrays, else the struct's scalars
    const int strategy = run_setting(sw.strategy, run, a.strategy), k = donors_of(strategy);
    const double F = run_setting(sw.F, run, a.F), CR = run_setting(sw.CR, run, a.CR);
    const bool repair = a.constraints != 0;
    int64_t d[kMaxDonors];
    int irand;
    philox_donors(P, k, row, grow, gen, key0, key1, n, d, irand);
    const double *__restrict__ gb = a.gbest + run * ld;
    double *__restrict__ out = a.pop2 + base + row * ld;
    const int nq = (n + LPR - 1) / LPR;
    for (int q0 = 0; q0 < nq; q0 += kStep) {  // four row steps per batch: one Philox call, loads in flight together
        double x[kStep], dv[kMaxDonors][kStep], g[kStep], r[kStep];
#pragma unroll
        for (int t = 0; t < kStep; ++t) {
            const int e = (q0 + t) * LPR + l;
            const bool in = e < n;
            x[t] = in ? xi[e] : 0.0;
            g[t] = in ? gb[e] : 0.0;
#pragma unroll
            for (int s = 0; s < kMaxDonors; ++s) dv[s][t] = (s < k && in) ? cur[d[s] * ld + e] : 0.0;
        }
#pragma unroll
        for (int t = 0; t < kStep; t += 2) {  // 53-bit crossover uniforms, the fused kernel's layout
            const U4 w = philox4x32_10((uint32_t)((q0 + t) >> 1) * (uint32_t)LPR + (uint32_t)l, grow, gen, kPurposeDeCross, key0,
                                       key1);
            r[t] = u53(w.x, w.y);
            r[t + 1] = u53(w.z, w.w);
        }
#pragma unroll
        for (int t = 0; t < kStep; ++t) {
            const int e = (q0 + t) * LPR + l;
            if (e >= n) continue;
            const double v = de_mutant(strategy, g[t], dv[0][t], dv[1][t], dv[2][t], dv[3][t], dv[4][t], F);
            double c = (e == irand || r[t] <= CR) ? v : x[t];  // de/_de.py:341-344
            if (repair && (c < a.lower[e] || c > a.upper[e]))  // de/_constraints.py:21-26
                c = a.lower[e] + (a.upper[e] - a.lower[e]) * philox_u53(e, LPR, grow, gen, kPurposeDeResample, key0, key1);
            out[e] = c;
        }
    }
}

// ---- 4. PSO: V = w*V + c1*r1*(pbest - X) + c2*r2*(gbest - X); X += V (after Shrink): X and V in place, per run
//      (pso_move_kernel's in-kernel-draw branch; the raw velocities wait in the workgroup's LDS for the row-wide beta)
template <int LPR>
__global__ __launch_bounds__(kMaxWavesPerBlock *kWave) void runs_pso_move_kernel(const sx_runs_rowwise_args a, const PsoSweep sw,
                                                                                 const int per_run) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int64_t run = (int64_t)blockIdx.x / per_run;
    const sx_state *st = a.state + run;
    if (st->done) return;
    const int n = a.n;
    const int64_t P = a.P, ld = n;
    const RowIds<LPR> id(P, (int)(run * per_run));
    const int l = id.l;
    const int64_t rowc = id.rowc, base = run * P * ld;
    double *Vn = lds + id.slot * (size_t)n;  // Shrink: the raw velocity waits here for the row-wide beta
    const uint32_t gen = (uint32_t)(st->it + 1), grow = (uint32_t)rowc;
    const uint32_t key0 = a.keys[2 * run], key1 = a.keys[2 * run + 1];
    double *xr = a.pop0 + base + rowc * ld, *vr = a.pop1 + base + rowc * ld;
    const double *pb = a.pop2 + base + rowc * ld, *gb = a.gbest + run * ld;
    const double w = run_setting(sw.w, run, a.w), c1 = run_setting(sw.c1, run, a.c1), c2 = run_setting(sw.c2, run, a.c2);
    const bool shrink = a.constraints != 0;
    double beta = __builtin_huge_val();
    const int nq = (n + LPR - 1) / LPR;
    for (int q0 = 0; q0 < nq; q0 += 2) {  // two row steps share one Philox call: 53-bit r1 / r2, the fused kernel's layout
        const U4 pw = philox4x32_10((uint32_t)(q0 >> 1) * (uint32_t)LPR + (uint32_t)l, grow, gen, kPurposePsoR1, key0, key1);
        const U4 pv = philox4x32_10((uint32_t)(q0 >> 1) * (uint32_t)LPR + (uint32_t)l, grow, gen, kPurposePsoR2, key0, key1);
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int e = (q0 + t) * LPR + l;
            if (e >= n) continue;
            const double v = vr[e], p = pb[e], g = gb[e], x = xr[e];
            const double r1 = t ? u53(pw.z, pw.w) : u53(pw.x, pw.y), r2 = t ? u53(pv.z, pv.w) : u53(pv.x, pv.y);
            const double vn = pso_velocity(w, v, c1, r1, p, x, c2, r2, g);
            if (shrink) {  // cpso/_constraints.py:22-50
                Vn[e] = vn;
                const double xc = x + vn, lo = a.lower[e], hi = a.upper[e];
                if (xc < lo) beta = fmin(beta, (lo - x) / vn);
                if (xc > hi) beta = fmin(beta, (hi - x) / vn);
            } else if (id.active) {
                vr[e] = vn;
                xr[e] = x + vn;
            }
        }
    }
    if (shrink) {
        beta = row_min<LPR>(beta);
        if (beta == __builtin_huge_val()) beta = 1.0;
        for (int e = l; e < n; e += LPR) {  // own elements only
            const double vn = Vn[e] * beta;
            if (id.active) {
                const double xn = xr[e] + vn;
                vr[e] = vn;
                xr[e] = xn;
            }
        }
    }
}

// ---- 5. selection_sync after the evaluation (_common.py:127-129), per run: rows_select_kernel's statements.  DE: the winner
//      or the old row into the other buffer; PSO: pbest in place; + the workgroup's best record
template <int LPR>
__global__ __launch_bounds__(kMaxWavesPerBlock *kWave) void runs_select_kernel(const sx_runs_rowwise_args a, const int per_run) {
    __shared__ double sf[kMaxRowsPerBlock];
    __shared__ int64_t si[kMaxRowsPerBlock];
    const int64_t run = (int64_t)blockIdx.x / per_run;
    const sx_state *st = a.state + run;
    if (st->done) return;
    const int n = a.n;
    const int64_t P = a.P, ld = n, base = run * P * ld, it = st->it;
    const RowIds<LPR> id(P, (int)(run * per_run));
    const double *__restrict__ f = a.f + run * P;
    double *__restrict__ xfun = a.fit + run * P, *__restrict__ candfit = a.candfit + run * P;
    const bool de = a.method == kDe;
    const double *cand = (de ? a.pop2 : a.pop0) + base;
    const double *xin = (de ? ((it & 1) ? a.pop1 : a.pop0) : a.pop2) + base;
    double *xout = (de ? ((it & 1) ? a.pop0 : a.pop1) : a.pop2) + base;
    const double fc = f[id.rowc], fold = xfun[id.rowc];
    const bool better = fc < fold;  // strict <
    if (id.active) {
        const double *src = better ? cand + id.row * ld : xin + id.row * ld;
        double *dst = xout + id.row * ld;
        if (better || xin != xout)
            for (int e = id.l; e < n; e += LPR) dst[e] = src[e];
        if (id.l == 0) {
            if (better) xfun[id.row] = fc;
            candfit[id.row] = fc;
        }
    }
    block_partial<LPR>(better ? fc : fold, id, sf, si, a.part_f + run * per_run, a.part_i + run * per_run);
}

// ---- 6. best of that generation, step of the best, status (_common.py:131-158): one workgroup per run,
//      select_finalize_kernel's statements (sx_core.hip) -- its dx in its order: thread t of 256 adds the squares of its
//      elements t, t + 256, ... in order, a wavefront's 64 sums meet in an xor butterfly (32 ... 1), the four wavefronts'
//      totals are added in order (dx <= xtol decides the status).  A run that ends leaves its results and counts itself
__global__ __launch_bounds__(kFinalWorkgroup) void runs_finalize_kernel(const sx_runs_rowwise_args a, const int per_run) {
    __shared__ double sf[kFinalWorkgroup / kWave];
    __shared__ int64_t si[kFinalWorkgroup / kWave];
    const int64_t run = blockIdx.x;
    sx_state *__restrict__ state = a.state + run;
    double bf = __builtin_huge_val();
    int64_t bi = INT64_MAX;
    scan_records(a.part_f + run * per_run, a.part_i + run * per_run, per_run, bf, bi);
    if (state->done) return;
    const int64_t it = state->it + 1;  // the generation being finalised
    block_argmin(bf, bi, sf, si);

    const int n = a.n;
    const int64_t base = run * a.P * n;
    double *__restrict__ gbest = a.gbest + run * n;
    const double *rows = a.method == kDe ? ((it & 1) ? a.pop1 : a.pop0) : a.pop2;
    const double *src = rows + base + bi * n;
    constexpr int kPer = (kWideFrom + kFinalWorkgroup - 1) / kFinalWorkgroup;
    double gv[kPer], sv[kPer];
    double acc = 0.0;
#pragma unroll
    for (int u = 0; u < kPer; ++u) {
        const int e = threadIdx.x + u * kFinalWorkgroup;
        gv[u] = e < n ? gbest[e] : 0.0;
        sv[u] = e < n ? src[e] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < kPer; ++u) {
        if (threadIdx.x + u * kFinalWorkgroup < n) {
            const double d = gv[u] - sv[u];
            acc += d * d;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, kWave);
    if ((threadIdx.x & 63) == 0) sf[threadIdx.x >> 6] = acc;
    __syncthreads();
    double ss = 0.0;
    for (int k = 0; k < kFinalWorkgroup / kWave; ++k) ss += sf[k];
    const double dx = sqrt(ss);
    int status = SX_STATUS_NONE;  // (every thread: the run's results below are written by all of them)
    if (dx <= a.xtol && bf <= a.ftol)
        status = 0;
    else if (bf <= a.ftol)
        status = 1;
    else if (it >= a.maxiter)
        status = -1;
    const bool over = status != SX_STATUS_NONE;
#pragma unroll
    for (int u = 0; u < kPer; ++u) {
        const int e = threadIdx.x + u * kFinalWorkgroup;
        if (e < n) {
            gbest[e] = sv[u];
            if (over) a.xs[run * n + e] = sv[u];
        }
    }
    if (threadIdx.x == 0) {
        state->it = it;
        state->gbidx = bi;
        state->gfit = bf;
        state->dx = dx;
        state->status = status;
        state->done = over;
        if (over) {
            a.funs[run] = bf;
            a.nits[run] = it;
            a.statuses[run] = status;
            atomicAdd(a.ended, 1);
        }
    }
}

// what every entry point checks (a->f, which may change from call to call, is checked where it is read); per_run <- records
// (= row workgroups) per run
int check_args(const sx_runs_rowwise_args *a, const char *who, int *per_run) {
    const std::string w(who);
    if (a == nullptr) {
        set_error(w + ": null args");
        return -1;
    }
    if (!(a->keys && a->lower && a->upper && a->pop0 && a->pop1 && a->pop2 && a->fit && a->candfit && a->state &&
          a->gbest && a->part_f && a->part_i && a->xs && a->funs && a->nits && a->statuses && a->ended)) {
        set_error(w + ": null device pointer");
        return -1;
    }
    if (!(a->R >= 1 && a->P >= 2 && a->n >= 1 && a->n <= kWideFrom && a->P < (int64_t)1 << 31 && a->R < (int64_t)1 << 31 &&
          a->R * a->P < (int64_t)1 << 31)) {
        set_error(w + ": bad shape (R >= 1, P >= 2, 1 <= n <= sx_wide_from(), R*P < 2^31)");
        return -1;
    }
    if (a->method != kDe && a->method != kPso) {
        set_error(w + ": unknown method");
        return -1;
    }
    if (a->constraints != 0 && a->constraints != 1) {
        set_error(w + ": unknown constraints");
        return -1;
    }
    if (a->x0 != nullptr && a->x0_stride != 0 && a->x0_stride != a->P * a->n) {
        set_error(w + ": bad x0 stride");
        return -1;
    }
    const int64_t each = sx_runs_rowwise_partials(a->P, a->n);
    if (each < 1 || a->R * each > (int64_t)INT32_MAX) {
        set_error(w + ": the grid of R * ceil(P / rows per workgroup) workgroups is beyond 2^31 - 1");
        return -1;
    }
    *per_run = (int)each;
    return 0;
}

}  // namespace

extern "C" int64_t sx_runs_rowwise_partials(int64_t P, int n) {
    if (P < 2 || n < 1 || n > kWideFrom) return -1;
    const int64_t rpb = rows_per_block(n);
    return (P + rpb - 1) / rpb;
}

extern "C" int sx_runs_rowwise_init(const sx_runs_rowwise_args *a, void *stream) {
    int per_run;
    if (check_args(a, "sx_runs_rowwise_init", &per_run)) return -1;
    const unsigned grid = (unsigned)(a->R * per_run), threads = (unsigned)(waves_per_block(a->n) * kWave);
    Enqueue q((hipStream_t)stream);
    SX_DISPATCH_LPR(a->n, return q.kernel(runs_init_kernel<LPR>, dim3(grid), dim3(threads), 0, *a, per_run))
    return -1;
}

extern "C" int sx_runs_rowwise_start(const sx_runs_rowwise_args *a, const int32_t *strategy, void *stream) {
    int per_run;
    if (check_args(a, "sx_runs_rowwise_start", &per_run)) return -1;
    SX_REQUIRE(a->f != nullptr, "sx_runs_rowwise_start: null objective values");
    Enqueue q((hipStream_t)stream);
    return q.kernel(runs_start_kernel, dim3((unsigned)a->R), dim3(kFinalWorkgroup), 0, *a, strategy);
}

extern "C" int sx_runs_rowwise_de_propose(const sx_runs_rowwise_args *a, const double *F, const double *CR,
                                          const int32_t *strategy, void *stream) {
    int per_run;
    if (check_args(a, "sx_runs_rowwise_de_propose", &per_run)) return -1;
    SX_REQUIRE(a->method == kDe, "sx_runs_rowwise_de_propose: the batch is not a DE batch");
    SX_REQUIRE(a->strategy >= 0 && a->strategy <= SX_DE_BEST2BIN, "sx_runs_rowwise_de_propose: unknown strategy");
    SX_REQUIRE(a->P - 1 >= donors_of(a->strategy), "sx_runs_rowwise_de_propose: population too small for the strategy");
    const unsigned grid = (unsigned)(a->R * per_run), threads = (unsigned)(waves_per_block(a->n) * kWave);
    const DeSweep sweep = {F, CR, strategy};
    Enqueue q((hipStream_t)stream);
    SX_DISPATCH_LPR(a->n, return q.kernel(runs_de_propose_kernel<LPR>, dim3(grid), dim3(threads), 0, *a, sweep, per_run))
    return -1;
}

extern "C" int sx_runs_rowwise_pso_move(const sx_runs_rowwise_args *a, const double *w, const double *c1, const double *c2,
                                        void *stream) {
    int per_run;
    if (check_args(a, "sx_runs_rowwise_pso_move", &per_run)) return -1;
    SX_REQUIRE(a->method == kPso, "sx_runs_rowwise_pso_move: the batch is not a PSO batch");
    const unsigned grid = (unsigned)(a->R * per_run), threads = (unsigned)(waves_per_block(a->n) * kWave);
    // Shrink's stash: a row of n doubles per row slot of the workgroup (at most 64 KiB: waves_per_block)
    const size_t lds = a->constraints != 0 ? (size_t)rows_per_block(a->n) * a->n * sizeof(double) : 0;
    const PsoSweep sweep = {w, c1, c2, nullptr};
    Enqueue q((hipStream_t)stream);
    SX_DISPATCH_LPR(a->n, return q.kernel(runs_pso_move_kernel<LPR>, dim3(grid), dim3(threads), lds, *a, sweep, per_run))
    return -1;
}

extern "C" int sx_runs_rowwise_select(const sx_runs_rowwise_args *a, void *stream) {
    int per_run;
    if (check_args(a, "sx_runs_rowwise_select", &per_run)) return -1;
    SX_REQUIRE(a->f != nullptr, "sx_runs_rowwise_select: null objective values");
    const unsigned grid = (unsigned)(a->R * per_run), threads = (unsigned)(waves_per_block(a->n) * kWave);
    Enqueue q((hipStream_t)stream);
    SX_DISPATCH_LPR(a->n, return q.kernel(runs_select_kernel<LPR>, dim3(grid), dim3(threads), 0, *a, per_run))
    return -1;
}

extern "C" int sx_runs_rowwise_finalize(const sx_runs_rowwise_args *a, void *stream) {
    int per_run;
    if (check_args(a, "sx_runs_rowwise_finalize", &per_run)) return -1;
    Enqueue q((hipStream_t)stream);
    return q.kernel(runs_finalize_kernel, dim3((unsigned)a->R), dim3(kFinalWorkgroup), 0, *a, per_run);
}
