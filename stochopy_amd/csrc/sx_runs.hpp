// The host tail the batched-runs kernels share (sx_de_runs.hip, sx_pso_runs.hip, sx_cma_runs.hip, sx_vd_runs.hip): one
// workgroup per run, its whole state in dynamic LDS.
#pragma once
#include <cstdint>

#include "sx_device.hpp"
#include "sx_enqueue.hpp"
#include "sx_rowops.hpp"  // SX_DISPATCH_FUN

namespace sx {

constexpr int64_t kLdsLimit = 160 * 1024;  // what one workgroup may declare on gfx950

// Per-run settings of a sweep (sx_*_runs_sweep_launch): DEVICE (R) arrays, element r for run r; a null pointer leaves the
// argument struct's scalar to every run.  A kernel takes its struct by value and picks once, at entry.
struct DeSweep {
    const double *F, *CR;
    const int32_t *strategy;
};
struct PsoSweep {
    const double *w, *c1, *c2, *gamma;
};
struct SigmaSweep {  // CMA-ES, VD-CMA
    const double *sigma;
};

template <class T>
__device__ __forceinline__ T run_setting(const T *per_run, int64_t run, T scalar) {
    return per_run != nullptr ? per_run[run] : scalar;
}

// R workgroups of `threads` threads with `lds` bytes of dynamic LDS each, onto `stream`
template <class Args, class Sweep>
__attribute__((visibility("hidden"))) int enqueue_runs(void (*kern)(const Args, const PlanArg, const Sweep), const Args &a,
                                                       const PlanArg &plan, const Sweep &sweep, int threads, int64_t lds,
                                                       void *stream) {
    if (lds > 64 * 1024)  // more than the default limit of dynamic LDS
        SX_HIP(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    Enqueue q((hipStream_t)stream);
    if (int rc = q.kernel(kern, dim3((unsigned)a.R), dim3((unsigned)threads), (size_t)lds, a, plan, sweep)) return rc;
    SX_LAUNCH_CHECK();
    return 0;
}

}  // namespace sx
