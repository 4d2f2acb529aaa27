// The host tail the batched-runs kernels share (sx_de_runs.hip, sx_pso_runs.hip, sx_cma_runs.hip, sx_vd_runs.hip): one
// workgroup per run, its whole state in dynamic LDS.
#pragma once
#include <cstdint>
#include <string>

#include "sx_device.hpp"
#include "sx_enqueue.hpp"
#include "sx_host.hpp"
#include "sx_rowops.hpp"  // SX_DISPATCH_FUN

namespace sx {

int make_plan_arg(int fun_id, int n, PlanArg *out);

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

// What the two sigma-swept launchers (sx_cma_runs_sweep_launch, sx_vd_runs_sweep_launch) check and prepare alike.
// The workspace is the runs' best-fitness histories, (R, maxiter) doubles; -1: no such launch
inline int64_t sigma_runs_workspace_bytes(int64_t R, int64_t maxiter) {
    if (R < 1 || maxiter < 1 || maxiter >= (int64_t)1 << 31 || R >= (int64_t)1 << 31) return -1;
    return R * maxiter * (int64_t)sizeof(double);
}
// who: the entry point's name for the messages (formed only when a check fails); [nmin, nmax]: its range of n; lds: its
// sx_*_runs_lds_bytes(P, n), does_not_fit: what it says when that is not positive.  A pointer that only one method has is
// that launcher's to check.  Leaves the objective's plan and the zero-initialised histories (stopping rules -5 and -7 read
// entries that no generation has written yet)
template <class Args>
__attribute__((visibility("hidden"))) int prepare_sigma_runs(const char *who, const Args *a, int nmin, int nmax, int64_t lds,
                                                             const char *does_not_fit, PlanArg *plan, void *stream) {
    SX_REQUIRE(a->keys && a->xmean0 && a->xm && a->xstd && a->w && a->work && a->xs && a->funs && a->nits && a->statuses,
               std::string(who) + ": null device pointer");
    SX_REQUIRE(a->R >= 1 && a->R < (int64_t)1 << 31 && a->P >= 2 && a->n >= nmin && a->n <= nmax && a->mu >= 1 &&
                   a->mu <= a->P && a->maxiter >= 1 && a->ilim >= 0,
               std::string(who) + ": bad shape");
    SX_REQUIRE(a->fun_id >= 0 && a->fun_id < SX_FUN_COUNT, std::string(who) + ": unknown objective");
    SX_REQUIRE(a->sigma > 0.0, std::string(who) + ": sigma must be positive");
    SX_REQUIRE(lds > 0, does_not_fit);
    if (make_plan_arg(a->fun_id, a->n, plan)) return -1;
    SX_HIP(hipMemsetAsync(a->work, 0, (size_t)sigma_runs_workspace_bytes(a->R, a->maxiter), (hipStream_t)stream));
    return 0;
}

}  // namespace sx
