// Many independent DE / PSO runs around a CALLER-SUPPLIED ROW-WISE objective: the batched counterpart of sx_unfused.hip
// (include/stochopy_hip.h, sx_runs_rowwise_args).  The objective cannot be fused, so the R populations live in device memory
// -- three (R, P, n) arrays -- and a generation of ALL runs is
//   propose / move kernel  ->  the caller's objective, ONCE, on the stacked (R*P, n) rows  ->  selection kernel  ->
//   one best / termination workgroup per run.
// The four steps of a generation are the single run's own (sx_unfused.hpp, where their reference code is listed): the kernels
// here find a workgroup's run, form that run's pointers, key and settings, and call them -- so given the same objective values
// run r is the single run of keys[r], bit for bit.  What only a batch has is written here: the initial populations, the start
// of every run, a run's results and the count of ended runs.
//
// Reference code replaced here (paths relative to the reference checkout), R times over:
//   stochopy/optimize/_common.py:109-120      the Latin hypercube (in-kernel draws: philox_lhs_element)
//   stochopy/optimize/de/_de.py:208-218       initial population and best
//   stochopy/optimize/cpso/_cpso.py:219-247   initial swarm (V = 0, pbest = X) and best
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
#include "sx_unfused.hpp"

using namespace sx;

namespace {

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

// ---- 3. DE: candidates of one generation -> cand, per run (de_propose_row with the run's key, settings and best row)
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
    const int64_t it = st->it, base = run * P * ld;
    // the run's own settings (uniform in the workgroup): element `run` of a sweep's arrays, else the struct's scalars
    de_propose_row<SX_RNG_PHILOX, LPR>(((it & 1) ? a.pop1 : a.pop0) + base, ld, P, n, id.l, id.row, (uint32_t)id.row,
                                       (uint32_t)(it + 1), a.keys[2 * run], a.keys[2 * run + 1],
                                       run_setting(sw.strategy, run, a.strategy), run_setting(sw.F, run, a.F),
                                       run_setting(sw.CR, run, a.CR), a.constraints != 0, a.lower, a.upper, a.gbest + run * ld,
                                       a.pop2 + base + id.row * ld, DeHostDraws{});
}

// ---- 4. PSO: X and V in place, per run (pso_move_row; with Shrink the raw velocities always wait in the workgroup's LDS)
template <int LPR>
__global__ __launch_bounds__(kMaxWavesPerBlock *kWave) void runs_pso_move_kernel(const sx_runs_rowwise_args a, const PsoSweep sw,
                                                                                 const int per_run) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int64_t run = (int64_t)blockIdx.x / per_run;
    const sx_state *st = a.state + run;
    if (st->done) return;
    const int n = a.n;
    const RowIds<LPR> id(a.P, (int)(run * per_run));
    const int64_t at = (run * a.P + id.rowc) * (int64_t)n;
    const bool shrink = a.constraints != 0;
    pso_move_row<SX_RNG_PHILOX, LPR>(a.pop0 + at, a.pop1 + at, a.pop2 + at, a.gbest + run * n, n, id.l, id.active,
                                     (uint32_t)id.rowc, (uint32_t)(st->it + 1), a.keys[2 * run], a.keys[2 * run + 1],
                                     run_setting(sw.w, run, a.w), run_setting(sw.c1, run, a.c1), run_setting(sw.c2, run, a.c2),
                                     shrink, a.lower, a.upper, lds + id.slot * (size_t)n, shrink, nullptr, nullptr);
}

// ---- 5. selection_sync after the evaluation, per run (rows_select_row).  DE: the winner or the old row into the other
//      buffer; PSO: pbest in place
template <int LPR>
__global__ __launch_bounds__(kMaxWavesPerBlock *kWave) void runs_select_kernel(const sx_runs_rowwise_args a, const int per_run) {
    const int64_t run = (int64_t)blockIdx.x / per_run;
    const sx_state *st = a.state + run;
    if (st->done) return;
    const int n = a.n;
    const int64_t P = a.P, base = run * P * n, it = st->it;
    const bool de = a.method == kDe;
    rows_select_row<LPR>(RowIds<LPR>(P, (int)(run * per_run)), (de ? a.pop2 : a.pop0) + base, n, a.f + run * P,
                         (de ? ((it & 1) ? a.pop1 : a.pop0) : a.pop2) + base, (de ? ((it & 1) ? a.pop0 : a.pop1) : a.pop2) + base,
                         n, a.fit + run * P, a.candfit + run * P, n, a.part_f + run * per_run, a.part_i + run * per_run);
}

// ---- 6. best of that generation, step of the best, status: one workgroup per run (best_step, as select_finalize_kernel of
//      sx_core.hip).  A run that ends leaves its results and counts itself
__global__ __launch_bounds__(kFinalWorkgroup) void runs_finalize_kernel(const sx_runs_rowwise_args a, const int per_run) {
    const int64_t run = blockIdx.x;
    sx_state *state = a.state + run;
    double bf = __builtin_huge_val();
    int64_t bi = INT64_MAX;
    scan_records(a.part_f + run * per_run, a.part_i + run * per_run, per_run, bf, bi);
    if (state->done) return;
    const int64_t it = state->it + 1;  // the generation being finalised
    const int n = a.n;
    const int64_t base = run * a.P * n;
    const bool de = a.method == kDe;
    double *gbest = a.gbest + run * n;
    const int status = best_step<(kWideFrom + kFinalWorkgroup - 1) / kFinalWorkgroup>(
        bf, bi, it, (de ? a.pop0 : a.pop2) + base, (de ? a.pop1 : a.pop2) + base, n, n, gbest, state, a.maxiter, a.xtol, a.ftol);
    if (status == SX_STATUS_NONE) return;
    for (int e = threadIdx.x; e < n; e += kFinalWorkgroup) a.xs[run * n + e] = gbest[e];  // (this thread's own stores)
    if (threadIdx.x == 0) {
        a.funs[run] = bf;
        a.nits[run] = it;
        a.statuses[run] = status;
        atomicAdd(a.ended, 1);
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
