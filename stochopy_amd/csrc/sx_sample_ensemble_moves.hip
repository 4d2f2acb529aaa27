// The ensemble sampler with several moves, a burn-in and thinning: sx_sample_ensemble.hip's run with the proposal of a sample
// chosen among up to four entries (kind, weight, parameter) -- the stretch move, the differential-evolution move (ter Braak 2006)
// and the snooker move (ter Braak & Vrugt 2008).  No counterpart in the reference.  include/stochopy_hip.h states the rule.
//
// Everything but the proposal is sx_sample_ensemble.hip's: replicas q = g W + w, the two half-sweeps, the LDS layout
//     X[W][n] the walkers | F[W] their values | U[rows][gen_row_stride(n)] one proposal staging area per row group
// (sx_sample_ensemble_lds_bytes), the passes of the row groups over the active half, the decision (chain_decide), the counters in
// the per-chain arrays of sx_sample_args.
//
// The move of sample it is ONE entry per ensemble (Philox slot 0, row g W, gen it, kPurposeSampleMove), so in the resident kernel
// the switch on its kind is uniform over the workgroup (every wave forms the entry from the same counter, by a ballot over the
// lanes that hold the entries and a readlane): every thread reaches both barriers of a sample, whatever the move.
//
// Hazards: as there.  An active row writes its own X[w], F[w] and U only and reads the INACTIVE half of X only -- one row of it
// under the stretch move, two under "de", three under "snooker" -- so the passes need no workgroup barrier and none is added.  The
// snooker move's two row sums (row_sum: shuffles within the row's own lanes) are taken by all lanes of an active row together.
//
// Recording: sample it goes to row (it - rec_start) / rec_every of xall / funall when it is one of rec_start, rec_start +
// rec_every, ...; the counters and the best values run over all samples.
#include "sx_sample_ensemble.hpp"

namespace sx {
int make_plan_arg(int fun_id, int n, PlanArg *out);

namespace {

// the entry of ensemble g at sample it: the first k with cum[k] > u, else the last.  Constant indices only: the struct stays in
// the kernel's argument segment
__device__ __forceinline__ void move_pick(const sx_sample_args &a, const sx_sample_ensemble_opts &mv, int64_t g, int W, int64_t it,
                                          int &kind, double &param) {
    kind = mv.kind[0], param = mv.param[0];
    if (mv.nmoves == 1) return;  // (cum[0] = 1.0 > u: no draw)
    const U4 w = philox4x32_10(0u, (uint32_t)(g * W), (uint32_t)it, kPurposeSampleMove, a.key0, a.key1);
    const double u = u53(w.x, w.y);
#pragma unroll
    for (int k = 3; k >= 0; --k) {
        const bool take = k < mv.nmoves && (k == mv.nmoves - 1 || mv.cum[k] > u);
        if (take) kind = mv.kind[k], param = mv.param[k];
    }
}

// "de" / "snooker": the indices of up to three distinct walkers within the other half (j3 only with `three`, which needs h >= 3)
// and d2
__device__ __forceinline__ void donors_draw(const sx_sample_args &a, uint32_t q, int64_t it, int h, bool three, int &j1, int &j2,
                                            int &j3, double &d2) {
    const U4 w0 = philox4x32_10(0u, q, (uint32_t)it, kPurposeSampleDonors, a.key0, a.key1);
    const U4 w1 = philox4x32_10(1u, q, (uint32_t)it, kPurposeSampleDonors, a.key0, a.key1);
    const double d0 = u53(w0.x, w0.y), d1 = u53(w0.z, w0.w);
    d2 = u53(w1.x, w1.y);
    j1 = (int)(d0 * (double)h);
    j1 = j1 < h - 1 ? j1 : h - 1;
    j2 = (int)(d1 * (double)(h - 1));
    j2 = j2 < h - 2 ? j2 : h - 2;
    j2 += j2 >= j1 ? 1 : 0;
    j3 = 0;
    if (three) {
        const int lo = j1 < j2 ? j1 : j2, hi = j1 < j2 ? j2 : j1;
        j3 = (int)(d2 * (double)(h - 2));
        j3 = j3 < h - 3 ? j3 : h - 3;
        j3 += j3 >= lo ? 1 : 0;
        j3 += j3 >= hi ? 1 : 0;
    }
}
__device__ __forceinline__ double de_gamma(double gamma0, double d2) { return gamma0 * (1.0 + 1e-5 * (2.0 * d2 - 1.0)); }

// The proposal of the active walker q (its row Xq) against the other half (its first row Xother) into U, by the lanes of the
// row; returns what the decision adds to fcur - f(Y).  Xq / Xother are LDS (resident) or device memory (around a caller's
// objective): the same expressions either way.
template <int LPR>
__device__ __forceinline__ double move_propose(const sx_sample_args &a, int kind, double param, uint32_t q, int64_t it, int h,
                                               const double *Xq, const double *Xother, double *U, int l, bool store) {
    const int n = a.n;
    if (kind == SX_ENSEMBLE_STRETCH) {
        int jj;
        double z;
        stretch_draw(a, q, it, h, param, jj, z);
        const double *Xj = Xother + (size_t)jj * n;
        for (int e = l; e < n; e += LPR) {
            const double xj = Xj[e];
            const double v = xj + z * (Xq[e] - xj);
            if (store) U[e] = v;
        }
        return stretch_factor(n, z);
    }
    int j1, j2, j3;
    double d2;
    donors_draw(a, q, it, h, kind == SX_ENSEMBLE_SNOOKER, j1, j2, j3, d2);
    const double *X1 = Xother + (size_t)j1 * n, *X2 = Xother + (size_t)j2 * n;
    if (kind == SX_ENSEMBLE_DE) {
        const double gamma = de_gamma(param, d2);
        for (int e = l; e < n; e += LPR) {
            const double v = Xq[e] + gamma * (X1[e] - X2[e]);
            if (store) U[e] = v;
        }
        return 0.0;
    }
    const double *X3 = Xother + (size_t)j3 * n;
    double dd = 0.0, pr = 0.0;
    for (int e = l; e < n; e += LPR) {
        const double delta = Xq[e] - X1[e];
        dd += delta * delta;
        pr += delta * (X2[e] - X3[e]);
    }
    dd = row_sum<LPR>(dd);
    pr = row_sum<LPR>(pr);
    double c = param * (pr / dd);
    if (!(dd > 0.0) || !(fabs(c) <= __DBL_MAX__)) c = 0.0;  // (a NaN c fails the comparison)
    for (int e = l; e < n; e += LPR) {
        const double xq = Xq[e];
        const double v = xq + c * (xq - X1[e]);
        if (store) U[e] = v;
    }
    return (double)(n - 1) * log(fabs(1.0 + c));
}

// thinning: is sample `it` recorded, and in which row of xall / funall (rec_every < 2^31, it < maxiter < 2^31)
__device__ __forceinline__ bool moves_record(const sx_sample_ensemble_opts &mv, int64_t it, int64_t &row) {
    row = 0;
    if (it < mv.rec_start) return false;
    const uint32_t off = (uint32_t)(it - mv.rec_start), every = (uint32_t)mv.rec_every;
    row = (int64_t)(off / every);
    return off % every == 0u;
}

template <int FUN, int LPR>
__global__ __launch_bounds__(kMaxWavesPerBlock *kWave) void ensemble_moves_kernel(const sx_sample_args a, const PlanArg plan, int W,
                                                                                  const sx_sample_ensemble_opts mv, int64_t it0,
                                                                                  int64_t it1) {
    extern __shared__ double lds[];
    constexpr int RPW = kWave / LPR;
    const int n = a.n, h = W / 2;
    const int tid = (int)threadIdx.x, nthreads = (int)blockDim.x;
    const int l = tid & (LPR - 1);
    const int slot = (tid >> 6) * RPW + (tid & 63) / LPR;
    const int rows = (nthreads >> 6) * RPW;
    const int64_t g = blockIdx.x;  // the ensemble
    const int64_t q0 = g * W;      // its first replica
    double *X = lds;
    double *F = X + (size_t)W * n;
    double *U = F + W + (size_t)slot * gen_row_stride(n);
    int64_t it = it0;
    if (it == 0) {  // sample 0: every walker's initial point (x0: one row per replica)
        const bool record = a.xall != nullptr && mv.rec_start == 0;
        for (int w0 = 0; w0 < W; w0 += rows) {
            const int w = w0 + slot;
            if (w < W) {
                const int64_t q = q0 + w;
                for (int e = l; e < n; e += LPR) U[e] = initial_value<LPR>(a, q, e);
                const double f0 = row_objective<FUN, LPR, 0, 0>(U, n, plan, l);
                double *all = record ? a.xall + ((g * mv.rec_rows) * W + w) * n : nullptr;
                for (int e = l; e < n; e += LPR) {
                    const double v = U[e];
                    X[w * n + e] = v;
                    a.xbest[q * n + e] = v;  // x = the first sample while nothing was accepted
                    if (record) st_stream(all + e, v);
                }
                if (l == 0) {
                    ChainState st;
                    st.start(f0);
                    st.store(a, q);
                    F[w] = f0;
                    if (record) st_stream(a.funall + (g * mv.rec_rows) * W + w, f0);
                }
            }
        }
        it = 1;
    } else {
        for (int i = tid; i < W * n; i += nthreads) X[i] = a.cur[q0 * n + i];
        for (int i = tid; i < W; i += nthreads) F[i] = a.fcur[q0 + i];
    }
    __syncthreads();
    // The entries wait in lanes 0 .. 3 of every wave (lane t: entry t) and the recording fields are narrowed to 32 bits: the
    // kernel is at the SGPR limit as sx_sample_ensemble.hip's is, and with the struct's 21 scalars live over the sample loop the
    // register allocator reserved a stack frame in one instantiation or another (profiles/sample_ensemble_moves_resources.txt
    // records scratch 0 for all of them: compare it after a change here)
    const int t = tid & 63;
    const int mykind = t == 0 ? mv.kind[0] : t == 1 ? mv.kind[1] : t == 2 ? mv.kind[2] : mv.kind[3];
    double mycum = t == 0 ? mv.cum[0] : t == 1 ? mv.cum[1] : t == 2 ? mv.cum[2] : mv.cum[3];
    // (the last entry always takes, the lanes behind it never)
    mycum = t < mv.nmoves - 1 ? mycum : t == mv.nmoves - 1 ? __builtin_huge_val() : -__builtin_huge_val();
    const double myparam = t == 0 ? mv.param[0] : t == 1 ? mv.param[1] : t == 2 ? mv.param[2] : mv.param[3];
    const bool draw = mv.nmoves > 1;
    const uint32_t rec_start = (uint32_t)mv.rec_start, rec_every = (uint32_t)mv.rec_every;  // (both < 2^31, as `it`)
    for (; it < it1; ++it) {
        // move_pick's rule: the first entry with cum > u, else the last (one entry: no draw).  A ballot and two readlanes: the
        // entry is a scalar, the branches on its kind below are uniform over the workgroup
        double u = 0.0;
        if (draw) {
            const U4 w = philox4x32_10(0u, (uint32_t)q0, (uint32_t)it, kPurposeSampleMove, a.key0, a.key1);
            u = u53(w.x, w.y);
        }
        const unsigned long long takes = __ballot(mycum > u);  // (never empty: lane nmoves - 1)
        const int k = __builtin_amdgcn_readfirstlane(__builtin_ctzll(takes));
        const int kind = __builtin_amdgcn_readlane(mykind, k);
        const double param = readlane_f64(myparam, k);
        const uint32_t rec_off = (uint32_t)it - rec_start;  // (wraps below rec_start: then not recorded)
        const bool record = a.xall != nullptr && (uint32_t)it >= rec_start && rec_off % rec_every == 0u;
        const int64_t rec_row = (int64_t)(rec_off / rec_every);
        for (int half = 0; half < 2; ++half) {
            const int abase = half * h, pbase = h - abase;  // the first walker of the active and of the other half
            for (int i0 = 0; i0 < h; i0 += rows) {
                const int i = i0 + slot;
                if (i < h) {
                    const int w = abase + i;
                    const int64_t q = q0 + w;
                    ChainState st;
                    st.load(a, q);
                    st.fcur = F[w];
                    double *Xq = X + w * n;
                    const double factor = move_propose<LPR>(a, kind, param, (uint32_t)q, it, h, Xq, X + pbase * n, U, l, true);
                    // (an infeasible proposal is evaluated too and its value dropped: the rows of a wave stay in step)
                    const double fY = row_objective<FUN, LPR, 0, 0>(U, n, plan, l);
                    const bool feasible = !a.reject || row_in_box<LPR>(a, U, n, l);
                    const double d = factor + (st.fcur - fY);
                    const Decision r = chain_decide(st, a, (uint32_t)q, it, true, feasible, d, fY);
                    // (each lane reads back the elements of U it wrote itself; the walker's state for this sample is final)
                    double *all = record ? a.xall + ((g * mv.rec_rows + rec_row) * W + w) * n : nullptr;
                    for (int e = l; e < n; e += LPR) {
                        const double v = r.accept ? U[e] : Xq[e];
                        if (r.accept) Xq[e] = v;
                        if (record) st_stream(all + e, v);
                        if (r.xbest_changed) a.xbest[q * n + e] = v;
                    }
                    if (l == 0) {
                        F[w] = st.fcur;
                        if (record) st_stream(a.funall + (g * mv.rec_rows + rec_row) * W + w, st.fcur);
                        st.store(a, q);
                    }
                }
            }
            __syncthreads();  // the half is complete: the next one reads it (and the row groups their walkers' counters)
        }
    }
    for (int i = tid; i < W * n; i += nthreads) a.cur[q0 * n + i] = X[i];
}

using ensemble_moves_kernel_t = void (*)(const sx_sample_args, const PlanArg, int, const sx_sample_ensemble_opts, int64_t, int64_t);

// ---- around a caller's objective ------------------------------------------------------------------------------------
// it = 0: prop (C W, n) = the initial points.  it >= 1: prop (C h, n) = the proposals of the active half, logzf (C h) what the
// decision adds to fcur - f(Y)
template <int LPR>
__global__ __launch_bounds__(kMaxWavesPerBlock *kWave) void ensemble_propose_moves_kernel(const sx_sample_args a, int W,
                                                                                          const sx_sample_ensemble_opts mv,
                                                                                          int64_t it, int half,
                                                                                          double *__restrict__ prop,
                                                                                          double *__restrict__ logzf) {
    const int n = a.n, h = W / 2;
    if (it == 0) {
        const RowIds<LPR> id(a.C);
        for (int e = id.l; e < n; e += LPR) {
            const double v = initial_value<LPR>(a, id.rowc, e);
            if (id.active) prop[id.rowc * n + e] = v;
        }
        return;
    }
    const RowIds<LPR> id((a.C / W) * h);
    const HalfRow r(id.rowc, W, half);
    int kind;
    double param;
    move_pick(a, mv, r.g, W, it, kind, param);
    const double *Xq = a.cur + r.q * n;
    const double *Xother = a.cur + (r.g * W + (h - half * h)) * n;
    const double factor = move_propose<LPR>(a, kind, param, (uint32_t)r.q, it, h, Xq, Xother, prop + id.rowc * n, id.l, id.active);
    if (id.active && id.l == 0) logzf[id.rowc] = factor;
}

// the decision on those proposals with their values fprop, and the walkers' bookkeeping (it = 0: fprop (C W) starts them)
template <int LPR>
__global__ __launch_bounds__(kMaxWavesPerBlock *kWave) void ensemble_decide_moves_kernel(const sx_sample_args a, int W,
                                                                                         const sx_sample_ensemble_opts mv,
                                                                                         int64_t it, int half,
                                                                                         const double *__restrict__ prop,
                                                                                         const double *__restrict__ fprop,
                                                                                         const double *__restrict__ logzf) {
    const int n = a.n, l = threadIdx.x & (LPR - 1);
    const RowIds<LPR> id(it == 0 ? a.C : (a.C / W) * (W / 2));
    const double *U = prop + id.rowc * n;
    const double fU = fprop[id.rowc];
    ChainState st;
    Decision r{true, true, 0.0};  // (sample 0: cur = the initial point)
    int64_t g, q;
    int w;
    if (it == 0) {
        q = id.rowc, g = q / W, w = (int)(q - g * W);
        st.start(fU);
    } else {
        const HalfRow hr(id.rowc, W, half);
        g = hr.g, q = hr.q, w = hr.w;
        st.load(a, q);
        const bool feasible = !a.reject || row_in_box<LPR>(a, U, n, l);
        r = chain_decide(st, a, (uint32_t)q, it, true, feasible, logzf[id.rowc] + (st.fcur - fU), fU);
    }
    if (!id.active) return;
    int64_t rec_row;
    const bool record = moves_record(mv, it, rec_row) && a.xall != nullptr;
    commit_sample<LPR>(a, st, q, l, U, r.accept, r.xbest_changed, record, (g * mv.rec_rows + rec_row) * W + w);
}

// what every *_moves entry point `who` requires of `mv` next to check_ensemble_args (which comes first: a is not null here)
inline int check_ensemble_opts(const char *who, const sx_sample_args *a, int W, const sx_sample_ensemble_opts *mv) {
    SX_SAMPLE_REQUIRE(mv != nullptr, "null move options");
    SX_SAMPLE_REQUIRE(mv->nmoves >= 1 && mv->nmoves <= 4, "nmoves outside [1, 4]");
    double below = 0.0;
    for (int k = 0; k < mv->nmoves; ++k) {
        const double p = mv->param[k];
        SX_SAMPLE_REQUIRE(mv->kind[k] == SX_ENSEMBLE_STRETCH || mv->kind[k] == SX_ENSEMBLE_DE || mv->kind[k] == SX_ENSEMBLE_SNOOKER,
                          "unknown move kind");
        SX_SAMPLE_REQUIRE(mv->cum[k] > below, "cum does not increase from 0");
        below = mv->cum[k];
        if (mv->kind[k] == SX_ENSEMBLE_STRETCH)
            SX_SAMPLE_REQUIRE(stretch_ok(p), "param of a stretch entry is not a finite number > 1");
        else
            SX_SAMPLE_REQUIRE(std::isfinite(p) && p > 0.0, "param of a de / snooker entry is not a finite number > 0");
        SX_SAMPLE_REQUIRE(mv->kind[k] != SX_ENSEMBLE_SNOOKER || W >= 6, "a snooker entry needs W >= 6 (three distinct walkers of a half)");
    }
    SX_SAMPLE_REQUIRE(below == 1.0, "cum does not end at 1.0");
    SX_SAMPLE_REQUIRE(mv->rec_start >= 0 && mv->rec_start <= a->maxiter - 1, "rec_start outside [0, maxiter - 1]");
    SX_SAMPLE_REQUIRE(mv->rec_every >= 1 && mv->rec_every < (int64_t)1 << 31, "rec_every outside [1, 2^31)");
    SX_SAMPLE_REQUIRE(mv->rec_rows == (a->maxiter - mv->rec_start + mv->rec_every - 1) / mv->rec_every,
                      "rec_rows is not ceil((maxiter - rec_start) / rec_every)");
    return 0;
}

}  // namespace
}  // namespace sx

using namespace sx;

extern "C" int sx_sample_ensemble_opts_bytes(void) { return (int)sizeof(sx_sample_ensemble_opts); }

extern "C" int sx_sample_ensemble_run_moves(const sx_sample_args *a, int W, const sx_sample_ensemble_opts *mv, int64_t it0,
                                            int64_t steps, void *stream) {
    const char *who = "sx_sample_ensemble_run_moves";
    if (check_ensemble_args(who, a, W, it0, steps, true)) return -1;
    if (check_ensemble_opts(who, a, W, mv)) return -1;
    if (steps == 0) return 0;
    PlanArg plan;
    if (make_plan_arg(a->fun_id, a->n, &plan)) return -1;
    ensemble_moves_kernel_t kern = nullptr;
    if (lanes_per_row(a->n) == 16) {
        SX_DISPATCH_FUN(a->fun_id, (kern = ensemble_moves_kernel<FUN, 16>))
    } else {  // (32: the 64-lane rows were refused above)
        SX_DISPATCH_FUN(a->fun_id, (kern = ensemble_moves_kernel<FUN, 32>))
    }
    const int lds = sx_sample_ensemble_lds_bytes(W, a->n);
    if (lds > 64 * 1024)  // more than the default limit (gfx950: 160 KiB per workgroup)
        SX_HIP(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    Enqueue q((hipStream_t)stream);
    return q.kernel(kern, dim3((unsigned)(a->C / W)), dim3(ensemble_waves(W, a->n) * kWave), (size_t)lds, *a, plan, W, *mv, it0,
                    it0 + steps);
}

extern "C" int sx_sample_ensemble_propose_moves(const sx_sample_args *a, int W, const sx_sample_ensemble_opts *mv, int64_t it,
                                                int half, double *prop, double *logzf, void *stream) {
    const char *who = "sx_sample_ensemble_propose_moves";
    if (check_ensemble_args(who, a, W, it, 1, false)) return -1;
    if (check_ensemble_opts(who, a, W, mv)) return -1;
    SX_SAMPLE_REQUIRE(prop != nullptr && (it == 0 || logzf != nullptr), "null proposal / factor array");
    SX_SAMPLE_REQUIRE(half == 0 || half == 1, "half is 0 or 1");
    const Geometry g = walker_geometry(it == 0 ? a->C : a->C / 2, a->n);
    Enqueue q((hipStream_t)stream);
    SX_DISPATCH_LPR(a->n, return q.kernel(ensemble_propose_moves_kernel<LPR>, dim3(g.blocks), dim3(g.threads), 0, *a, W, *mv, it,
                                          half, prop, logzf))
    return -1;
}

extern "C" int sx_sample_ensemble_decide_moves(const sx_sample_args *a, int W, const sx_sample_ensemble_opts *mv, int64_t it,
                                               int half, const double *prop, const double *fprop, const double *logzf,
                                               void *stream) {
    const char *who = "sx_sample_ensemble_decide_moves";
    if (check_ensemble_args(who, a, W, it, 1, false)) return -1;
    if (check_ensemble_opts(who, a, W, mv)) return -1;
    SX_SAMPLE_REQUIRE(prop != nullptr && fprop != nullptr && (it == 0 || logzf != nullptr), "null proposal / value / factor array");
    SX_SAMPLE_REQUIRE(half == 0 || half == 1, "half is 0 or 1");
    const Geometry g = walker_geometry(it == 0 ? a->C : a->C / 2, a->n);
    Enqueue q((hipStream_t)stream);
    SX_DISPATCH_LPR(a->n, return q.kernel(ensemble_decide_moves_kernel<LPR>, dim3(g.blocks), dim3(g.threads), 0, *a, W, *mv, it, half,
                                          prop, fprop, logzf))
    return -1;
}
