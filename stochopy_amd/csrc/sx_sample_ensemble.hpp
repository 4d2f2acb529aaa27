// What the two translation units of the ensemble sampler share (sx_sample_ensemble.hip: the stretch move alone;
// sx_sample_ensemble_moves.hip: several moves, burn-in and thinning): the shape of an ensemble's workgroup, the stretch draw, the
// rows of a half-sweep around a caller's objective, and the host checks of sx_sample_args.
#pragma once
#include <cmath>

#include "sx_enqueue.hpp"
#include "sx_host.hpp"
#include "sx_rowops.hpp"
#include "sx_sample.hpp"

namespace sx {
namespace {

constexpr size_t kEnsembleLds = 160 * 1024;  // what a workgroup may declare (gfx950); the kernel has no static LDS

// waves of an ensemble's workgroup: as many as give rows >= h, up to the caps
inline int ensemble_waves(int W, int n) {
    const int rpw = kWave / lanes_per_row(n);
    const int cap = kMaxRowsPerBlock / rpw < kMaxWavesPerBlock ? kMaxRowsPerBlock / rpw : kMaxWavesPerBlock;
    const int need = (W / 2 + rpw - 1) / rpw;
    return need < cap ? need : cap;
}
inline bool ensemble_shape(int W, int n) { return n >= 1 && n <= kWideFrom && W >= 4 && W % 2 == 0 && W / 2 >= n; }

// the stretch of walker q at sample it: the partner's index within the other half and z
__device__ __forceinline__ void stretch_draw(const sx_sample_args &a, uint32_t q, int64_t it, int h, double stretch, int &jj,
                                             double &z) {
    const U4 w = philox4x32_10(0u, q, (uint32_t)it, kPurposeSampleStretch, a.key0, a.key1);
    const double d0 = u53(w.x, w.y), d1 = u53(w.z, w.w);
    jj = (int)(d0 * (double)h);
    jj = jj < h - 1 ? jj : h - 1;
    const double t = (stretch - 1.0) * d1 + 1.0;
    z = (t * t) / stretch;
}
// what the decision adds to fcur - f(Y)
__device__ __forceinline__ double stretch_factor(int n, double z) { return (double)(n - 1) * log(z); }

// ---- around a caller's objective ------------------------------------------------------------------------------------
inline Geometry walker_geometry(int64_t rows, int n) {
    const int waves = waves_per_workgroup(n, 0);
    const int rpb = waves * (kWave / lanes_per_row(n));
    return Geometry{(unsigned)((rows + rpb - 1) / rpb), (unsigned)(waves * kWave), 0};
}

// row r of a half-sweep's (C h) rows: walker half h + r % h of ensemble r / h
struct HalfRow {
    int64_t g, q;
    int w;
    __device__ __forceinline__ HalfRow(int64_t r, int W, int half) {
        const int h = W / 2;
        g = r / h;
        w = half * h + (int)(r - g * h);
        q = g * W + w;
    }
};

// What every ensemble entry point `who` requires of sx_sample_args before it launches samples [it0, it0 + steps): the sibling of
// check_sample_args for method = SX_SAMPLE_ENSEMBLE (step, k, nleap, jac, fd_step, normals and logu are not read).  `resident`:
// the objective is compiled into the kernel and the ensemble lives in LDS.
inline int check_ensemble_args(const char *who, const sx_sample_args *a, int W, int64_t it0, int64_t steps, bool resident) {
    SX_SAMPLE_REQUIRE(a != nullptr, "null args");
    SX_SAMPLE_REQUIRE(a->cur && a->fcur && a->facc && a->fmin && a->xbest && a->iacc && a->imin && a->nacc && a->nfeas,
                      "null state pointer");
    SX_SAMPLE_REQUIRE(a->lower && a->upper, "bounds missing");
    SX_SAMPLE_REQUIRE(a->method == SX_SAMPLE_ENSEMBLE, "method is not SX_SAMPLE_ENSEMBLE");
    SX_SAMPLE_REQUIRE(a->C >= 1 && a->C < (int64_t)1 << 31 && ensemble_shape(W, a->n) && a->C % W == 0,
                      "bad shape (W even, >= 4 and >= 2 n; C = ensembles x W replicas)");
    SX_SAMPLE_REQUIRE(!resident || (a->fun_id >= 0 && a->fun_id < SX_FUN_COUNT), "unknown objective");
    SX_SAMPLE_REQUIRE(a->rng == SX_RNG_PHILOX, "the draws are made in the kernels (SX_RNG_PHILOX)");
    SX_SAMPLE_REQUIRE(a->maxiter >= 1 && a->maxiter < (int64_t)1 << 31 && it0 >= 0 && steps >= 0 && it0 + steps <= a->maxiter,
                      "samples outside [0, maxiter)");
    SX_SAMPLE_REQUIRE((a->xall == nullptr) == (a->funall == nullptr), "xall and funall go together");
    SX_SAMPLE_REQUIRE(a->x0 == nullptr || a->x0_stride >= a->n, "x0 is one row per replica");
    if (resident) {
        const int lds = sx_sample_ensemble_lds_bytes(W, a->n);
        SX_SAMPLE_REQUIRE(lds > 0 && (size_t)lds <= kEnsembleLds, "the ensemble does not fit the LDS of a workgroup");
    }
    return 0;
}
inline bool stretch_ok(double stretch) { return std::isfinite(stretch) && stretch > 1.0; }

}  // namespace
}  // namespace sx
