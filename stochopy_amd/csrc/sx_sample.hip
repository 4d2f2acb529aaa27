// Samplers (stochopy/sample): Metropolis-Hastings and Hamiltonian Monte-Carlo with many independent chains.
//
// A Markov chain is sequential, independent chains never talk to each other: one row group (lanes_per_row(n) lanes)
// carries ONE chain for the whole launch.  The chain's rows -- current sample, proposal / position, momentum and the two
// finite-difference copies -- live in that row group's slice of LDS, its scalars (current value, best values, counts)
// in registers; there is no workgroup barrier, no grid barrier and no exchange.  A launch advances every chain by
// `it1 - it0` samples and writes row i of xall / funall with streaming stores as it goes.  State that has to survive
// from launch to launch (a run with a callback is one launch per sample) round-trips through sx_sample_args' per-chain
// arrays unchanged, so cutting a run into launches does not change a bit of it.
//
// Draws: SX_RNG_HOST reads the reference's own stream from memory (normals, log of the acceptance uniform: the order
// does not depend on the data as long as nothing is rejected for feasibility); SX_RNG_PHILOX keys every draw by
// (slot, chain, sample, purpose) -- sx_device.hpp kPurposeSample* -- so a chain depends on its index and the key only.
//
// The kernel templates are in sx_sample_kernels.hpp: this file instantiates the plain and the adapting form, sx_sample_metric.hip
// the form with per-axis scales.  The two resident kernels keep their OWN spelling of the chain step (proposal, decision, load / record / store), the
// one sx_sample.hpp states for the unfused and tempered kernels: folded into those shared functions the same arithmetic came out
// 1 - 3 % slower here (register allocation and scheduling of the sample loop moved), so the copies stay and the
// GPU tests hold the two spellings together bit for bit (tests/test_gpu_sample_batched.py, test_gpu_sample_temper.py).
#include "sx_enqueue.hpp"
#include "sx_host.hpp"
#include "sx_rowops.hpp"
#include "sx_sample.hpp"
#include "sx_sample_kernels.hpp"

namespace sx {
namespace {

template <int FUN, int LPR>
__global__ __launch_bounds__(kMaxWavesPerBlock *kWave) void gradient_kernel(const double *__restrict__ Xg, int64_t P, int n,
                                                                            double *__restrict__ G) {
    extern __shared__ double lds[];
    const RowIds<LPR> id(P);
    const int l = id.l;
    double *Q = lds + (size_t)id.slot * n;
    for (int e = l; e < n; e += LPR) Q[e] = Xg[id.rowc * n + e];
    lds_wave_fence();
    const bool active = id.active;
    double *g = G + id.rowc * n;
    grad_apply<FUN, LPR>(Q, n, l, [&](int e, double gv) {
        if (active) g[e] = gv;
    });
}

}  // namespace
}  // namespace sx

using namespace sx;

extern "C" int sx_sample_chains_per_workgroup(int method, int jac, int n) {
    if (n < 1 || n > kWideFrom) return -1;
    return sample_waves(variant_of(method, jac), n) * (kWave / lanes_per_row(n));
}

extern "C" int sx_sample_run(const sx_sample_args *a, int64_t it0, int64_t steps, void *stream) {
    return run_chains<false>("sx_sample_run", a, nullptr, nullptr, it0, steps, stream);
}

extern "C" int sx_sample_adapt_bytes(void) { return (int)sizeof(sx_sample_adapt); }

extern "C" int sx_sample_run_adapt(const sx_sample_args *a, const sx_sample_adapt *ad, int64_t it0, int64_t steps,
                                   void *stream) {
    return run_chains<true>("sx_sample_run_adapt", a, ad, nullptr, it0, steps, stream);
}

extern "C" int sx_sample_gradient(int fun_id, const double *X, int64_t P, int n, double *G, void *stream) {
    SX_REQUIRE(X && G && P >= 1 && n >= 1 && n <= kWideFrom, "sx_sample_gradient: bad arguments");
    SX_REQUIRE(fun_id >= 0 && fun_id < SX_FUN_COUNT, "sx_sample_gradient: unknown objective");
    const int waves = waves_per_workgroup(n, (size_t)n * sizeof(double));
    const int rows = waves * (kWave / lanes_per_row(n));
    Enqueue q((hipStream_t)stream);
    SX_DISPATCH_LPR(n, SX_DISPATCH_FUN(fun_id, return q.kernel(gradient_kernel<FUN, LPR>, dim3((unsigned)((P + rows - 1) / rows)),
                                                               dim3(waves * kWave), (size_t)rows * n * sizeof(double), X, P, n, G)))
    return -1;
}
