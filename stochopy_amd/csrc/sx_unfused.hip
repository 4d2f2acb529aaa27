// Generations around a CALLER-SUPPLIED objective (backend hook contract: a callable that maps the
// (P, n) device array to (P,) fitness values).  The objective cannot be fused, so a generation is
//   propose / move kernel  ->  caller's objective on the device array  ->  selection kernel  ->  sx_select_finalize
// with the same draws, arithmetic and record layout as the fused kernels: given bit-identical fitness values the
// run is the fused run, bit for bit.
//
// The steps themselves -- and the reference code they replace -- are in sx_unfused.hpp, shared with the batched runs
// (sx_runs_unfused.hip); the kernels here form ONE run's pointers and settings out of sx_de_args / sx_pso_args and call them.
// Reference: stochopy/optimize/_common.py:27-106, the population wrapper `fun(X)`, is the caller's callable.
#include "sx_device.hpp"
#include "sx_host.hpp"
#include "sx_rowops.hpp"
#include "sx_unfused.hpp"

using namespace sx;

namespace {

// candidates of one generation -> cand (P, n) row-major; nothing else is touched
template <int RNG, int LPR>
__global__ __launch_bounds__(kMaxWavesPerBlock *kWave) void de_propose_kernel(const sx_de_args a,
                                                                              double *__restrict__ cand) {
    const sx_state *st = a.state;
    if (st->done) return;
    const RowIds<LPR> id(a.P);
    if (!id.active) return;
    const int64_t it = st->it;
    const double *cur = (it & 1) ? a.buf1 : a.buf0;
    const double *gb = a.gbest != nullptr ? a.gbest : cur + st->gbidx * a.ld;
    de_propose_row<RNG, LPR>(cur, a.ld, a.P, a.n, id.l, id.row, (uint32_t)(a.row0 + id.row), (uint32_t)(it + 1), a.key0, a.key1,
                             a.strategy, a.F, a.CR, a.constraints != 0, a.lower, a.upper, gb, cand + id.row * (int64_t)a.n,
                             DeHostDraws{a.r1, a.resample, a.donors, a.irand});
}

// X and V of one generation in place.  has_stash: the launch brought rows_per_block(n) * n doubles of dynamic LDS (not for
// wide rows, n > kWideFrom: pso_move_row's form without a stash)
template <int RNG, int LPR>
__global__ __launch_bounds__(kMaxWavesPerBlock *kWave) void pso_move_kernel(const sx_pso_args a, const int has_stash) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const sx_state *st = a.state;
    if (st->done) return;
    const int n = a.n;
    const RowIds<LPR> id(a.P);
    const int64_t at = id.rowc * a.ld, draws = id.rowc * (int64_t)n;
    const bool shrink = a.constraints != 0;
    pso_move_row<RNG, LPR>(a.X + at, a.V + at, a.pbest + at, a.gbest, n, id.l, id.active, (uint32_t)(a.row0 + id.rowc),
                           (uint32_t)(st->it + 1), a.key0, a.key1, a.w, a.c1, a.c2, shrink, a.lower, a.upper,
                           lds + id.slot * (size_t)n, shrink && has_stash, RNG == SX_RNG_HOST ? a.r1 + draws : nullptr,
                           RNG == SX_RNG_HOST ? a.r2 + draws : nullptr);
}

template <int LPR>
__global__ __launch_bounds__(kMaxWavesPerBlock *kWave) void rows_select_kernel(
    const double *__restrict__ cand, int64_t ldc, const double *__restrict__ f, const double *xin, double *xout,
    int64_t ldx, double *__restrict__ xfun, double *__restrict__ candfit, int64_t P, int n, const sx_state *st,
    double *__restrict__ part_f, int64_t *__restrict__ part_i) {
    if (st->done) return;
    rows_select_row<LPR>(RowIds<LPR>(P), cand, ldc, f, xin, xout, ldx, xfun, candfit, n, part_f, part_i);
}

}  // namespace

extern "C" int sx_de_propose(const sx_de_args *a, double *cand, void *stream) {
    SX_REQUIRE(a != nullptr && cand != nullptr, "sx_de_propose: null pointer");
    SX_REQUIRE(a->buf0 && a->buf1 && a->state, "sx_de_propose: null device pointer");
    SX_REQUIRE(a->P >= 2 && a->P < (int64_t)1 << 31 && a->n >= 1 && a->ld >= a->n, "sx_de_propose: bad shape");
    SX_REQUIRE(a->strategy >= 0 && a->strategy <= SX_DE_BEST2BIN, "sx_de_propose: unknown strategy");
    SX_REQUIRE(a->P - 1 >= donors_of(a->strategy), "sx_de_propose: population too small for the strategy");
    SX_REQUIRE(a->rng == SX_RNG_HOST || a->rng == SX_RNG_PHILOX, "sx_de_propose: unknown rng mode");
    SX_REQUIRE(a->rng != SX_RNG_HOST || (a->r1 && a->donors && a->irand), "sx_de_propose: host draws missing");
    SX_REQUIRE(a->constraints == 0 || (a->lower && a->upper && (a->rng != SX_RNG_HOST || a->resample)),
               "sx_de_propose: bounds / resample draws missing");
    const Geometry g = row_geometry(a->P, a->n, run_wide_from(a->wide_from));
    if (a->rng == SX_RNG_PHILOX) {
        SX_DISPATCH_LPR(a->n, hipLaunchKernelGGL((de_propose_kernel<SX_RNG_PHILOX, LPR>), dim3(g.blocks), dim3(g.threads), 0,
                                                 (hipStream_t)stream, *a, cand))
    } else {
        SX_DISPATCH_LPR(a->n, hipLaunchKernelGGL((de_propose_kernel<SX_RNG_HOST, LPR>), dim3(g.blocks), dim3(g.threads), 0,
                                                 (hipStream_t)stream, *a, cand))
    }
    SX_LAUNCH_CHECK();
    return 0;
}

extern "C" int sx_pso_move(const sx_pso_args *a, void *stream) {
    SX_REQUIRE(a != nullptr, "sx_pso_move: null args");
    SX_REQUIRE(a->X && a->V && a->pbest && a->gbest && a->state, "sx_pso_move: null device pointer");
    SX_REQUIRE(a->P >= 2 && a->n >= 1 && a->ld >= a->n, "sx_pso_move: bad shape");
    SX_REQUIRE(a->rng == SX_RNG_HOST || a->rng == SX_RNG_PHILOX, "sx_pso_move: unknown rng mode");
    SX_REQUIRE(a->rng != SX_RNG_HOST || (a->r1 && a->r2), "sx_pso_move: host draws missing");
    SX_REQUIRE(a->constraints == 0 || (a->lower && a->upper), "sx_pso_move: bounds missing");
    const Geometry g = row_geometry(a->P, a->n, kWideFrom);
    const size_t lds = a->n > kWideFrom ? 0 : (size_t)rows_per_block(a->n) * a->n * sizeof(double);
    if (a->rng == SX_RNG_PHILOX) {
        SX_DISPATCH_LPR(a->n, hipLaunchKernelGGL((pso_move_kernel<SX_RNG_PHILOX, LPR>), dim3(g.blocks), dim3(g.threads), lds,
                                                 (hipStream_t)stream, *a, lds != 0 ? 1 : 0))
    } else {
        SX_DISPATCH_LPR(a->n, hipLaunchKernelGGL((pso_move_kernel<SX_RNG_HOST, LPR>), dim3(g.blocks), dim3(g.threads), lds,
                                                 (hipStream_t)stream, *a, lds != 0 ? 1 : 0))
    }
    SX_LAUNCH_CHECK();
    return 0;
}

extern "C" int sx_rows_select(const double *cand, int64_t ldc, const double *f, const double *xin, double *xout,
                              int64_t ldx, double *xfun, double *candfit, int64_t P, int n, const sx_state *state,
                              double *part_f, int64_t *part_i, void *stream) {
    SX_REQUIRE(cand && f && xin && xout && xfun && state && part_f && part_i, "sx_rows_select: null pointer");
    SX_REQUIRE(P >= 1 && n >= 1 && ldc >= n && ldx >= n, "sx_rows_select: bad shape");
    const Geometry g = row_geometry(P, n, kWideFrom);
    SX_DISPATCH_LPR(n, hipLaunchKernelGGL((rows_select_kernel<LPR>), dim3(g.blocks), dim3(g.threads), 0, (hipStream_t)stream,
                                          cand, ldc, f, xin, xout, ldx, xfun, candfit, P, n, state, part_f, part_i))
    SX_LAUNCH_CHECK();
    return 0;
}
