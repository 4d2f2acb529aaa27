// The affine-invariant ensemble sampler (Goodman & Weare 2010, the stretch move): ENSEMBLES of W device-resident walkers.
// No counterpart in the reference.
//
// Walker w of ensemble g is replica q = g W + w: q takes the chain index's place in every draw and in the per-chain arrays of
// sx_sample_args, which are C W long.  h = W / 2.  Sample 0 is the initial state.  Sample it >= 1 is two half-sweeps: in half 0
// the walkers [0, h) are active and read the walkers [h, W); in half 1 the walkers [h, W) are active and read [0, h), which
// half 0 has already updated.  The active walker q makes ONE Philox call (slot 0, row q, gen it, kPurposeSampleStretch):
//     d0 = u53(w.x, w.y):  partner j = base + min(h - 1, (int)(d0 * h)), base the first walker of the other half
//     d1 = u53(w.z, w.w):  z = ((a - 1) * d1 + 1)^2 / a, a = `stretch`
//     Y[e] = X_j[e] + z * (X_q[e] - X_j[e]);   d = (n - 1) * log(z) + (fcur_q - f(Y))
// and the decision is the samplers' own (sx_sample.hpp chain_decide: box test with reject, the acceptance draw of (q, it),
// min(0, d) > log u, a NaN d accepts; the best values by ChainState::accept, the mcmc rule).
//
// Layout of the resident kernel: one workgroup per ensemble, one launch per run.  LDS of the workgroup:
//     X[W][n] the walkers | F[W] their values | U[rows][gen_row_stride(n)] one proposal staging area per row group
// A workgroup has as many waves as give rows >= h row groups, up to the row kernels' caps (kMaxWavesPerBlock waves,
// kMaxRowsPerBlock rows); where h is larger the row groups walk the active half in passes (walker base + p rows + slot in pass p:
// a walker always meets the same row group).  W >= 2 n must fit the LDS, so only rows of up to 128 elements (16 / 32 lanes) occur.
//
// Hazards: within a half-sweep an active row writes its own X[w], F[w] and U only and reads the INACTIVE half of X only, so the
// passes need no workgroup barrier -- the wave fence of row_objective around a row's own U is all.  One __syncthreads() after
// each half-sweep; every thread of the workgroup reaches both (the sample, half and pass loops are uniform over the workgroup;
// idle row groups and the rows of a ragged last pass skip the work, not the barrier).
//
// A walker's counters (facc, iacc, fmin, imin, nacc, nfeas) live in the per-chain arrays of sx_sample_args between its
// decisions, not in LDS: W >= 2 n bounds what an ensemble may take of the LDS (7 W more doubles would lower the largest W), they
// go back to those arrays at the end of a launch anyway, a run cut into launches is then the same run by construction, and the
// decide kernel around a caller's objective below reads them in the same place.  A walker is loaded and stored by its own
// row group (all lanes load, lane 0 stores), a barrier apart.  fcur is read from F.
//
// Around a CALLER-SUPPLIED objective (factory.batched) a half-sweep is propose kernel -> objective on the (C h, n) proposals ->
// decide kernel, the walkers in device memory (a.cur), one row group per active walker; same draws, same expressions under
// -ffp-contract=off: with bit-identical objective values it is the resident run, bit for bit.  These kernels serve every row
// length the samplers serve (no LDS).
#include "sx_sample_ensemble.hpp"

namespace sx {
int make_plan_arg(int fun_id, int n, PlanArg *out);

namespace {

template <int FUN, int LPR>
__global__ __launch_bounds__(kMaxWavesPerBlock *kWave) void ensemble_kernel(const sx_sample_args a, const PlanArg plan, int W,
                                                                            double stretch, int64_t it0, int64_t it1) {
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
    const bool record = a.xall != nullptr;
    int64_t it = it0;
    if (it == 0) {  // sample 0: every walker's initial point (x0: one row per replica)
        for (int w0 = 0; w0 < W; w0 += rows) {
            const int w = w0 + slot;
            if (w < W) {
                const int64_t q = q0 + w;
                for (int e = l; e < n; e += LPR) U[e] = initial_value<LPR>(a, q, e);
                const double f0 = row_objective<FUN, LPR, 0, 0>(U, n, plan, l);
                double *all = record ? a.xall + ((g * a.maxiter) * W + w) * n : nullptr;
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
                    if (record) st_stream(a.funall + (g * a.maxiter) * W + w, f0);
                }
            }
        }
        it = 1;
    } else {
        for (int i = tid; i < W * n; i += nthreads) X[i] = a.cur[q0 * n + i];
        for (int i = tid; i < W; i += nthreads) F[i] = a.fcur[q0 + i];
    }
    __syncthreads();
    for (; it < it1; ++it) {
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
                    int jj;
                    double z;
                    stretch_draw(a, (uint32_t)q, it, h, stretch, jj, z);
                    double *Xq = X + w * n;
                    const double *Xj = X + (pbase + jj) * n;
                    for (int e = l; e < n; e += LPR) {
                        const double xj = Xj[e];
                        U[e] = xj + z * (Xq[e] - xj);
                    }
                    // (an infeasible proposal is evaluated too and its value dropped: the rows of a wave stay in step)
                    const double fY = row_objective<FUN, LPR, 0, 0>(U, n, plan, l);
                    const bool feasible = !a.reject || row_in_box<LPR>(a, U, n, l);
                    const double d = stretch_factor(n, z) + (st.fcur - fY);
                    const Decision r = chain_decide(st, a, (uint32_t)q, it, true, feasible, d, fY);
                    // (each lane reads back the elements of U it wrote itself; the walker's state for this sample is final)
                    double *all = record ? a.xall + ((g * a.maxiter + it) * W + w) * n : nullptr;
                    for (int e = l; e < n; e += LPR) {
                        const double v = r.accept ? U[e] : Xq[e];
                        if (r.accept) Xq[e] = v;
                        if (record) st_stream(all + e, v);
                        if (r.xbest_changed) a.xbest[q * n + e] = v;
                    }
                    if (l == 0) {
                        F[w] = st.fcur;
                        if (record) st_stream(a.funall + (g * a.maxiter + it) * W + w, st.fcur);
                        st.store(a, q);
                    }
                }
            }
            __syncthreads();  // the half is complete: the next one reads it (and the row groups their walkers' counters)
        }
    }
    for (int i = tid; i < W * n; i += nthreads) a.cur[q0 * n + i] = X[i];
}

using ensemble_kernel_t = void (*)(const sx_sample_args, const PlanArg, int, double, int64_t, int64_t);

// ---- around a caller's objective (walker_geometry, HalfRow: sx_sample_ensemble.hpp) ------------------------------------
// it = 0: prop (C W, n) = the initial points.  it >= 1: prop (C h, n) = the proposals of the active half, logzf (C h) their
// factors (n - 1) log z
template <int LPR>
__global__ __launch_bounds__(kMaxWavesPerBlock *kWave) void ensemble_propose_kernel(const sx_sample_args a, int W, double stretch,
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
    int jj;
    double z;
    stretch_draw(a, (uint32_t)r.q, it, h, stretch, jj, z);
    const double *Xq = a.cur + r.q * n;
    const double *Xj = a.cur + (r.g * W + (h - half * h) + jj) * n;
    double *U = prop + id.rowc * n;
    for (int e = id.l; e < n; e += LPR) {
        const double xj = Xj[e];
        const double v = xj + z * (Xq[e] - xj);
        if (id.active) U[e] = v;
    }
    if (id.active && id.l == 0) logzf[id.rowc] = stretch_factor(n, z);
}

// the decision on those proposals with their values fprop, and the walkers' bookkeeping (it = 0: fprop (C W) starts them)
template <int LPR>
__global__ __launch_bounds__(kMaxWavesPerBlock *kWave) void ensemble_decide_kernel(const sx_sample_args a, int W, int64_t it,
                                                                                   int half, const double *__restrict__ prop,
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
    commit_sample<LPR>(a, st, q, l, U, r.accept, r.xbest_changed, a.xall != nullptr, (g * a.maxiter + it) * W + w);
}

}  // namespace
}  // namespace sx

using namespace sx;

// 8 (W n + W + rows gen_row_stride(n)) bytes, rows = RPW * min(cap, ceil(W / 2 / RPW)) row groups with RPW = 64 /
// lanes_per_row(n) rows per wave and cap = min(kMaxWavesPerBlock, kMaxRowsPerBlock / RPW) waves; -1 unless W is even, >= 4 and
// >= 2 n and n is a row of 16 or 32 lanes (1 <= n <= 128)
extern "C" int sx_sample_ensemble_lds_bytes(int W, int n) {
    if (!ensemble_shape(W, n) || lanes_per_row(n) == kWave || W > (1 << 20)) return -1;
    const int rows = ensemble_waves(W, n) * (kWave / lanes_per_row(n));
    const int64_t bytes = (int64_t)sizeof(double) * ((int64_t)W * n + W + (int64_t)rows * gen_row_stride(n));
    return bytes < ((int64_t)1 << 31) ? (int)bytes : -1;
}

extern "C" int sx_sample_ensemble_run(const sx_sample_args *a, int W, double stretch, int64_t it0, int64_t steps, void *stream) {
    const char *who = "sx_sample_ensemble_run";
    if (check_ensemble_args(who, a, W, it0, steps, true)) return -1;
    SX_SAMPLE_REQUIRE(stretch_ok(stretch), "stretch is not a finite number > 1");
    if (steps == 0) return 0;
    PlanArg plan;
    if (make_plan_arg(a->fun_id, a->n, &plan)) return -1;
    ensemble_kernel_t kern = nullptr;
    if (lanes_per_row(a->n) == 16) {
        SX_DISPATCH_FUN(a->fun_id, (kern = ensemble_kernel<FUN, 16>))
    } else {  // (32: the 64-lane rows were refused above)
        SX_DISPATCH_FUN(a->fun_id, (kern = ensemble_kernel<FUN, 32>))
    }
    const int lds = sx_sample_ensemble_lds_bytes(W, a->n);
    if (lds > 64 * 1024)  // more than the default limit (gfx950: 160 KiB per workgroup)
        SX_HIP(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    Enqueue q((hipStream_t)stream);
    return q.kernel(kern, dim3((unsigned)(a->C / W)), dim3(ensemble_waves(W, a->n) * kWave), (size_t)lds, *a, plan, W, stretch, it0,
                    it0 + steps);
}

extern "C" int sx_sample_ensemble_propose(const sx_sample_args *a, int W, double stretch, int64_t it, int half, double *prop,
                                          double *logzf, void *stream) {
    const char *who = "sx_sample_ensemble_propose";
    if (check_ensemble_args(who, a, W, it, 1, false)) return -1;
    SX_SAMPLE_REQUIRE(stretch_ok(stretch), "stretch is not a finite number > 1");
    SX_SAMPLE_REQUIRE(prop != nullptr && (it == 0 || logzf != nullptr), "null proposal / factor array");
    SX_SAMPLE_REQUIRE(half == 0 || half == 1, "half is 0 or 1");
    const Geometry g = walker_geometry(it == 0 ? a->C : a->C / 2, a->n);
    Enqueue q((hipStream_t)stream);
    SX_DISPATCH_LPR(a->n, return q.kernel(ensemble_propose_kernel<LPR>, dim3(g.blocks), dim3(g.threads), 0, *a, W, stretch, it, half,
                                          prop, logzf))
    return -1;
}

extern "C" int sx_sample_ensemble_decide(const sx_sample_args *a, int W, int64_t it, int half, const double *prop,
                                         const double *fprop, const double *logzf, void *stream) {
    const char *who = "sx_sample_ensemble_decide";
    if (check_ensemble_args(who, a, W, it, 1, false)) return -1;
    SX_SAMPLE_REQUIRE(prop != nullptr && fprop != nullptr && (it == 0 || logzf != nullptr), "null proposal / value / factor array");
    SX_SAMPLE_REQUIRE(half == 0 || half == 1, "half is 0 or 1");
    const Geometry g = walker_geometry(it == 0 ? a->C : a->C / 2, a->n);
    Enqueue q((hipStream_t)stream);
    SX_DISPATCH_LPR(a->n, return q.kernel(ensemble_decide_kernel<LPR>, dim3(g.blocks), dim3(g.threads), 0, *a, W, it, half, prop, fprop,
                                          logzf))
    return -1;
}
