// What the CMA-ES and VD-CMA kernels say alike, once: the ordered stopping rules, the facts they are decided on and the
// workgroup reduction that gathers them.  Plain device functions: values in, no flag that selects a caller.
// Callers: cma_stop_kernel (sx_cma_loop.hip), vd_update_kernel and the wide chain's phases G and H (sx_vd_loop.hip):
// everything that applies to them; vd_runs_kernel (sx_vd_runs.hip): reduce_many, rule_facts_add, history_extremes.
// The two batched kernels sit at their register limits and keep, on measurement, their own spelling of the rest
// (vd_runs_kernel: cma_stop_status; cma_runs_kernel, sx_cma_runs.hip: all of it) under comments that name the function
// here: A CORRECTION MADE HERE IS OWED THERE.
//
// Reference code stated here (paths relative to the reference checkout):
//   stochopy/optimize/cmaes/_cmaes.py:360-434   converge: the ten ordered rules, incl. the reads of the zero-initialised
//                                               history
#pragma once
#include <cstdint>

#include "sx_device.hpp"

namespace sx {

// ---- K values at once (kind[q]: 0 sum, 1 max, 2 min)
template <int K>
__device__ __forceinline__ double fold_kind(const int (&kind)[K], int q, double u, double v) {
    return kind[q] == 0 ? u + v : (kind[q] == 1 ? fmax(u, v) : fmin(u, v));
}
// over the 64 lanes of a wavefront: an xor butterfly (32 ... 1), every lane gets the results
template <int K>
__device__ __forceinline__ void wave_reduce_many(double (&v)[K], const int (&kind)[K]) {
#pragma unroll
    for (int q = 0; q < K; ++q) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v[q] = fold_kind(kind, q, v[q], __shfl_xor(v[q], off, kWave));
    }
}
// over a workgroup of NW wavefronts: one pair of barriers for all K, the wavefronts' totals folded in order by every
// thread; red: NW * K doubles of LDS, which the next call may reuse at once
template <int K, int NW>
__device__ __forceinline__ void reduce_many(double (&v)[K], const int (&kind)[K], double *red) {
    wave_reduce_many(v, kind);
    __syncthreads();  // (the previous reduction's readers are through)
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int q = 0; q < K; ++q) red[(threadIdx.x >> 6) * K + q] = v[q];
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < K; ++q) {
        double r = red[q];
        for (int wv = 1; wv < NW; ++wv) r = fold_kind(kind, q, r, red[wv * K + q]);
        v[q] = r;
    }
}
template <int NW>
__device__ __forceinline__ double reduce_one(double x, int how, double *red) {
    double v[1] = {x};
    const int k[1] = {how};
    reduce_many<1, NW>(v, k, red);
    return v[0];
}

// ---- the best-fitness histories of rules -5 and -7, this thread's share (thread tid of nthreads): the window
//      [gen - ilim, gen] of the zero-initialised array hist[maxiter] -- entry `gen` is read before it is written, as in
//      the reference -- into wmax, wmin; the whole array joined with this generation's fit[P] into jmax, jmin
template <class I>
__device__ __forceinline__ void history_extremes(const double *hist, const double *fit, I gen, I ilim, I maxiter, I P, I tid,
                                                 I nthreads, double &wmax, double &wmin, double &jmax, double &jmin) {
    wmax = -__builtin_inf(), wmin = __builtin_inf(), jmax = -__builtin_inf(), jmin = __builtin_inf();
    if (gen >= ilim) {
        const I hi = gen + 1 < maxiter ? gen + 1 : maxiter;
        for (I k = gen - ilim + tid; k < hi; k += nthreads) {
            const double v = hist[k];
            wmax = fmax(wmax, v), wmin = fmin(wmin, v);
        }
    }
    for (I k = tid; k < maxiter; k += nthreads) {
        const double v = hist[k];
        jmax = fmax(jmax, v), jmin = fmin(jmin, v);
    }
    for (I k = tid; k < P; k += nthreads) {
        const double v = fit[k];
        jmax = fmax(jmax, v), jmin = fmin(jmin, v);
    }
}

// ---- what one dimension adds to the facts of rules -3, -6 and -8: sd = sqrt(C_ee), pc_e its element of the path.
//      "any(x)" is a count, "all(x < t)" the count of elements that FAIL (NaN fails, as in numpy)
__device__ __forceinline__ void rule_facts_add(double sd, double sigma, double insigma, double pc_e, double &any_small,
                                               double &any_large, double &nan_sd, double &sdmax, double &fail_pc) {
    if (0.2 * sigma * sd < 1.0e-10) any_small += 1.0;
    if (sigma * sd > 1.0e3 * insigma) any_large += 1.0;
    if (sd != sd) nan_sd += 1.0;
    sdmax = fmax(sdmax, sd);
    if (!(sigma * fabs(pc_e) < 1.0e-11 * insigma)) fail_pc += 1.0;
}

// VD-CMA has no B, D: rules -2 and -4 cannot fire with these in fail_axis and nan_d
constexpr double kRuleOff = 1.0;

// ---- the ordered rules (:360-434), from the reduced facts; SX_STATUS_NONE: go on.  I: the caller's integer type of a
//      generation number.
//      dx2 |xmean - xold|^2, fbest this generation's best;  fail_axis: elements that fail rule -2's all(...) on the axis of
//      this generation;  any_small, any_large, nan_sd, sdmax, fail_pc: rule_facts_add;  nan_d, dmax, dmin: of D (rule -4 is
//      off when D holds a NaN: numpy's max / min propagate it and the comparison is False);  wmax ... jmin: history_extremes
template <class I>
__device__ __forceinline__ int cma_stop_status(I gen, I maxiter, I ilim, double xtol, double ftol, double sigma, double insigma,
                                               double dx2, double fbest, double fail_axis, double any_small, double nan_d,
                                               double dmax, double dmin, double wmax, double wmin, double any_large, double jmax,
                                               double jmin, double fail_pc, double nan_sd, double sdmax) {
    int status = SX_STATUS_NONE;
    if (gen >= maxiter)
        status = -1;
    else if (sqrt(dx2) <= xtol && fbest < ftol)
        status = 0;
    else if (fbest <= ftol)
        status = 1;
    else if (fail_axis == 0.0)
        status = -2;
    else if (any_small > 0.0)
        status = -3;
    else if (nan_d == 0.0 && dmax > 1.0e7 * dmin)
        status = -4;
    else if (gen >= ilim && wmax - wmin < 1.0e-10)
        status = -5;
    else if (any_large > 0.0)
        status = -6;
    else if (gen > 2 && jmax - jmin < 1.0e-12)
        status = -7;
    else if (fail_pc == 0.0 && nan_sd == 0.0 && sigma * sdmax < 1.0e-11 * insigma)
        status = -8;
    return status;
}

}  // namespace sx
