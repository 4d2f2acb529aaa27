// The four steps of a DE / PSO generation around a CALLER-SUPPLIED objective, each stated once: the proposal of a row, the
// move of a row, the selection of a row with its workgroup's record, the best / termination step of one workgroup.
// sx_unfused.hip (one run) and sx_runs_unfused.hip (R runs) call them with their own pointers and settings; sx_core.hip's
// select_finalize_kernel calls the last one.  Values and pointers go in, no flag names a caller: run r of a batch is the
// single run of its key bit for bit because both execute these statements.
//
// Reference code replaced (paths relative to the reference checkout):
//   stochopy/optimize/de/_de.py:314-351       de_sync up to the candidates U (mutation, crossover, Random)
//   stochopy/optimize/cpso/_cpso.py:324-329   mutation (velocity / position) + cpso/_constraints.py:4-53
//   stochopy/optimize/_common.py:123-130      selection_sync after `candfun = fun(cand)`: strict <, in place
//   stochopy/optimize/_common.py:131-158      argmin + the termination ladder (sync_status, sx_rowops.hpp)
#pragma once
#include "sx_device.hpp"
#include "sx_rowops.hpp"

namespace sx {

constexpr int kProposeStep = 4;  // row steps per batch of the DE proposal

// the draws of a host-rng DE generation (sx_de_args); read only under RNG == SX_RNG_HOST
struct DeHostDraws {
    const double *r1, *resample;  // (P, n)
    const int32_t *donors;        // (k, P)
    const int32_t *irand;         // (P)
};

// DE: the candidate of row `row` of the population `cur` (P rows, stride ld) -> out[0..n); nothing else is touched.
// grow: the row's global number (the Philox counters), gb: the best row
template <int RNG, int LPR>
__device__ __forceinline__ void de_propose_row(const double *__restrict__ cur, int64_t ld, int64_t P, int n, int l, int64_t row,
                                               uint32_t grow, uint32_t gen, uint32_t key0, uint32_t key1, int strategy, double F,
                                               double CR, bool repair, const double *lower, const double *upper,
                                               const double *__restrict__ gb, double *__restrict__ out, const DeHostDraws &h) {
    const double *__restrict__ xi = cur + row * ld;
    const int k = donors_of(strategy);
    int64_t d[kMaxDonors];
    int irand;
    if (RNG == SX_RNG_PHILOX) {
        philox_donors(P, k, row, grow, gen, key0, key1, n, d, irand);
    } else {
#pragma unroll
        for (int t = 0; t < kMaxDonors; ++t) d[t] = t < k ? (int64_t)h.donors[(int64_t)t * P + row] : 0;
        irand = h.irand[row];
    }
    constexpr int kStep = kProposeStep;
    const int nq = (n + LPR - 1) / LPR;
    for (int q0 = 0; q0 < nq; q0 += kStep) {  // four row steps per batch: one Philox call, loads in flight together
        double x[kStep], dv[kMaxDonors][kStep], g[kStep], r[kStep], rs[kStep];
#pragma unroll
        for (int t = 0; t < kStep; ++t) {
            const int e = (q0 + t) * LPR + l;
            const bool in = e < n;
            x[t] = in ? xi[e] : 0.0;
            g[t] = in ? gb[e] : 0.0;
#pragma unroll
            for (int s = 0; s < kMaxDonors; ++s) dv[s][t] = (s < k && in) ? cur[d[s] * ld + e] : 0.0;
            r[t] = (RNG == SX_RNG_HOST && in) ? h.r1[row * (int64_t)n + e] : 2.0;
            rs[t] = (RNG == SX_RNG_HOST && in && repair) ? h.resample[row * (int64_t)n + e] : 0.0;
        }
        if (RNG == SX_RNG_PHILOX) {
#pragma unroll
            for (int t = 0; t < kStep; t += 2) {  // 53-bit crossover uniforms, the fused kernel's layout
                const U4 w = philox4x32_10((uint32_t)((q0 + t) >> 1) * (uint32_t)LPR + (uint32_t)l, grow, gen, kPurposeDeCross,
                                           key0, key1);
                r[t] = u53(w.x, w.y);
                r[t + 1] = u53(w.z, w.w);
            }
        }
#pragma unroll
        for (int t = 0; t < kStep; ++t) {
            const int e = (q0 + t) * LPR + l;
            if (e >= n) continue;
            const double v = de_mutant(strategy, g[t], dv[0][t], dv[1][t], dv[2][t], dv[3][t], dv[4][t], F);
            double c = (e == irand || r[t] <= CR) ? v : x[t];  // de/_de.py:341-344
            if (repair && (c < lower[e] || c > upper[e]))      // de/_constraints.py:21-26
                c = RNG == SX_RNG_HOST
                        ? rs[t]
                        : lower[e] + (upper[e] - lower[e]) * philox_u53(e, LPR, grow, gen, kPurposeDeResample, key0, key1);
            out[e] = c;
        }
    }
}

// PSO: V = w*V + c1*r1*(pbest - X) + c2*r2*(gbest - X); X += V (after Shrink) of one row, X and V in place.  xr, vr, pb (and
// r1, r2: this row of the host draws, read only under RNG == SX_RNG_HOST) are the row's own; a padding row (!active) runs
// along and stores nothing.  Shrink needs the row-wide beta before any element moves: with `stash` the raw velocities wait
// for it in Vn (the row's n doubles of LDS); without -- wide rows: one wavefront per row, no dynamic LDS -- they are formed
// AGAIN behind beta: same operands, same operations, same bits
template <int RNG, int LPR>
__device__ __forceinline__ void pso_move_row(double *xr, double *vr, const double *pb, const double *gb, int n, int l, bool active,
                                             uint32_t grow, uint32_t gen, uint32_t key0, uint32_t key1, double w, double c1,
                                             double c2, bool shrink, const double *lower, const double *upper, double *Vn,
                                             bool stash, const double *r1row, const double *r2row) {
    double beta = __builtin_huge_val();
    const int nq = (n + LPR - 1) / LPR;
    // raw velocity of the two elements (q0 + t) * LPR + l, t = 0, 1 (one Philox call)
    auto raw = [&](int q0, double(&x)[2], double(&vn)[2]) {
        U4 pw = {0u, 0u, 0u, 0u}, pv = {0u, 0u, 0u, 0u};  // 53-bit r1 / r2, the fused kernel's layout
        if (RNG == SX_RNG_PHILOX) {
            pw = philox4x32_10((uint32_t)(q0 >> 1) * (uint32_t)LPR + (uint32_t)l, grow, gen, kPurposePsoR1, key0, key1);
            pv = philox4x32_10((uint32_t)(q0 >> 1) * (uint32_t)LPR + (uint32_t)l, grow, gen, kPurposePsoR2, key0, key1);
        }
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int e = (q0 + t) * LPR + l;
            x[t] = 0.0, vn[t] = 0.0;
            if (e >= n) continue;
            const double v = vr[e], p = pb[e], g = gb[e];
            x[t] = xr[e];
            double r1 = t ? u53(pw.z, pw.w) : u53(pw.x, pw.y), r2 = t ? u53(pv.z, pv.w) : u53(pv.x, pv.y);
            if (RNG == SX_RNG_HOST) {
                r1 = r1row[e];
                r2 = r2row[e];
            }
            vn[t] = pso_velocity(w, v, c1, r1, p, x[t], c2, r2, g);
        }
    };
    for (int q0 = 0; q0 < nq; q0 += 2) {  // two row steps share one Philox call
        double x[2], vn[2];
        raw(q0, x, vn);
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int e = (q0 + t) * LPR + l;
            if (e >= n) continue;
            if (shrink) {  // cpso/_constraints.py:22-50
                if (stash) Vn[e] = vn[t];
                const double xc = x[t] + vn[t], lo = lower[e], hi = upper[e];
                if (xc < lo) beta = fmin(beta, (lo - x[t]) / vn[t]);
                if (xc > hi) beta = fmin(beta, (hi - x[t]) / vn[t]);
            } else if (active) {
                vr[e] = vn[t];
                xr[e] = x[t] + vn[t];
            }
        }
    }
    if (!shrink) return;
    beta = row_min<LPR>(beta);
    if (beta == __builtin_huge_val()) beta = 1.0;
    if (stash) {
        for (int e = l; e < n; e += LPR) {  // own elements only
            const double vn = Vn[e] * beta;
            if (active) {
                const double xn = xr[e] + vn;
                vr[e] = vn;
                xr[e] = xn;
            }
        }
    } else {
        for (int q0 = 0; q0 < nq; q0 += 2) {
            double x[2], vn[2];
            raw(q0, x, vn);
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const int e = (q0 + t) * LPR + l;
                if (e >= n || !active) continue;
                const double vb = vn[t] * beta;
                vr[e] = vb;
                xr[e] = x[t] + vb;
            }
        }
    }
}

// selection_sync after the evaluation (_common.py:127-129): a row with f < xfun takes the candidate; xout may be xin (in
// place: PSO's pbest) or the other population buffer (DE); candfit may be null.  + the workgroup's best record
template <int LPR>
__device__ __forceinline__ void rows_select_row(const RowIds<LPR> &id, const double *__restrict__ cand, int64_t ldc,
                                                const double *__restrict__ f, const double *xin, double *xout, int64_t ldx,
                                                double *__restrict__ xfun, double *__restrict__ candfit, int n,
                                                double *__restrict__ part_f, int64_t *__restrict__ part_i) {
    __shared__ double sf[kMaxRowsPerBlock];
    __shared__ int64_t si[kMaxRowsPerBlock];
    const double fc = f[id.rowc], fold = xfun[id.rowc];
    const bool better = fc < fold;  // strict <
    if (id.active) {
        const double *src = better ? cand + id.row * ldc : xin + id.row * ldx;
        double *dst = xout + id.row * ldx;
        if (better || xin != xout)
            for (int e = id.l; e < n; e += LPR) dst[e] = src[e];
        if (id.l == 0) {
            if (better) xfun[id.row] = fc;
            if (candfit != nullptr) candfit[id.row] = fc;
        }
    }
    block_partial<LPR>(better ? fc : fold, id, sf, si, part_f, part_i);
}

// Best of generation `it` and termination (_common.py:131-158), one workgroup of kFinalWorkgroup threads for rows of up to
// kPer * kFinalWorkgroup elements.  (bf, bi): what this thread found in the workgroups' records (scan_records) -> the best
// of them all.  Generation g lives in rows[g & 1] (double-buffered populations); rows0 == rows1 for in-place state.
// dx = ||gbest - x[bi]||_2 (np.linalg.norm, _common.py:135), all loads of a thread in flight together, in an order that
// does not depend on kPer: thread t adds the squares of its elements t, t + 256, ... in order, a wavefront's 64 sums meet in
// an xor butterfly (32 ... 1), the four wavefronts' totals are added in order.  Then x[bi] -> gbest, and the state.
// Every thread returns the status
template <int kPer>
__device__ __forceinline__ int best_step(double &bf, int64_t &bi, int64_t it, const double *rows0, const double *rows1,
                                         int64_t ld, int n, double *__restrict__ gbest, sx_state *__restrict__ state, int maxiter,
                                         double xtol, double ftol) {
    __shared__ double sf[kFinalWorkgroup / kWave];
    __shared__ int64_t si[kFinalWorkgroup / kWave];
    block_argmin(bf, bi, sf, si);
    const double *src = ((it & 1) ? rows1 : rows0) + bi * ld;
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
#pragma unroll
    for (int u = 0; u < kPer; ++u)
        if (threadIdx.x + u * kFinalWorkgroup < n) gbest[threadIdx.x + u * kFinalWorkgroup] = sv[u];
    const int status = sync_status(dx, xtol, bf, ftol, it, maxiter);
    if (threadIdx.x == 0) {
        state->it = it;
        state->gbidx = bi;
        state->gfit = bf;
        state->dx = dx;
        state->status = status;
        state->done = status != SX_STATUS_NONE;
    }
    return status;
}

}  // namespace sx
