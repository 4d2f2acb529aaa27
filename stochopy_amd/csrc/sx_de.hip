// Differential Evolution: one fused kernel per generation
// (donor gather -> mutation -> binomial crossover -> bound repair -> objective
//  -> greedy selection -> per-workgroup best), plus the hipGraph of generations.
//
// Reference code replaced (paths relative to the reference checkout):
//   stochopy/optimize/de/_de.py:304-311   delete_shuffle_sync (donor indices)
//   stochopy/optimize/de/_de.py:314-351   de_sync
//   stochopy/optimize/de/_strategy.py:1-38  rand1bin / rand2bin / best1bin / best2bin
//   stochopy/optimize/de/_constraints.py:13-28  Random
//   stochopy/optimize/_common.py:123-130  selection (strict <, in place)
//   stochopy/factory/benchmark.py         objective, fused
//
// 16/32/64 lanes per individual (sx_rowops.hpp); the population is double-buffered: generation g
// lives in buf[g & 1], its successor is written to the other buffer (winner or
// unchanged row), so donor reads never race with selection writes.
#define SX_DE_XM 0
#include "sx_de_kernel.hpp"
#include "sx_wide.hpp"

namespace sx {
// the chained (sx_de_chain.hip) and peer-exchange (sx_de_p2p.hip) kernels, as launchable function pointers
de_kernel_t de_chain_kernel(int fun_id, int n, int64_t P, int strategy, int constraints);
de_kernel_t de_p2p_kernel(int fun_id, int n, int64_t P, int strategy, int constraints);
}

namespace {

int check_args(const sx_de_args *a) {
    SX_REQUIRE(a != nullptr, "sx_de: null args");
    SX_REQUIRE(a->buf0 && a->buf1 && a->fit && a->state && a->part_f && a->part_i, "sx_de: null device pointer");
    SX_REQUIRE(a->P >= 2 && a->P < (int64_t)1 << 31 && a->n >= 1 && a->ld >= a->n, "sx_de: bad shape");
    SX_REQUIRE(a->fun_id >= 0 && a->fun_id < SX_FUN_COUNT, "sx_de: unknown objective");
    SX_REQUIRE(a->strategy >= 0 && a->strategy <= 3, "sx_de: unknown strategy");
    SX_REQUIRE(a->P - 1 >= donors_of(a->strategy), "sx_de: popsize too small for the strategy");
    SX_REQUIRE(a->rng == SX_RNG_HOST || a->rng == SX_RNG_PHILOX, "sx_de: unknown rng mode");
    if (a->rng == SX_RNG_HOST) {
        SX_REQUIRE(a->r1 && a->donors && a->irand, "sx_de: host draws missing");
        SX_REQUIRE(a->constraints == 0 || a->resample, "sx_de: resample block missing");
    }
    SX_REQUIRE(a->constraints == 0 || (a->lower && a->upper), "sx_de: bounds missing");
    SX_REQUIRE(a->spec_store >= 0 && a->spec_store <= 3, "sx_de: spec_store must be 0 ... 3");
    return 0;
}

de_kernel_t kernel_for(const sx_de_args *a) {
    return a->rng == SX_RNG_PHILOX ? pick_kernel<SX_RNG_PHILOX, 0>(a->fun_id, a->n, a->P, a->strategy, a->constraints)
                                   : pick_kernel<SX_RNG_HOST, 0>(a->fun_id, a->n, a->P, a->strategy, a->constraints);
}

Geometry geometry(const sx_de_args *a) {
    Geometry g = row_geometry(a->P, a->n, de_wide_from(a));
    // rows of up to 256 elements stage nothing but the trial vector (sx_device.hpp gen_row_stride)
    if (!is_wide(a->n, de_wide_from(a))) g.lds = (size_t)rows_per_block(a->n) * gen_row_stride(a->n) * sizeof(double);
    return g;
}

// One generation: the generation kernel (rows of more than the run's wide_from elements: one workgroup per row, sx_wide.hip,
// one record per row) and, with `finalize`, the best / termination step behind it.  Every launch is identical (the
// per-generation state is read from a.state on the device), so a graph of generations is this, ngen times.
int enqueue_de_generation(Enqueue &q, const sx_de_args *a, int finalize) {
    const Geometry g = geometry(a);
    if (is_wide(a->n, de_wide_from(a))) {
        if (int rc = wide_de_enqueue(q, a)) return rc;
    } else {
        PlanArg plan;
        if (make_plan_arg(a->fun_id, a->n, &plan)) return -1;
        if (int rc = q.kernel(kernel_for(a), dim3(g.blocks), dim3(g.threads), g.lds, nullptr, nullptr, nullptr, g.blocks, *a,
                              plan, 0, 0, sx_xchg_args{}))
            return rc;
    }
    if (!finalize) return 0;
    SX_REQUIRE(a->gbest != nullptr, "sx_de_generation: the separate finalize kernel needs the gbest buffer");
    return enqueue_finalize(q, a->part_f, a->part_i, g.blocks, a->buf0, a->buf1, a->ld, a->n, a->gbest, a->state, a->maxiter,
                            a->xtol, a->ftol);
}

}  // namespace

extern "C" int sx_de_generation(const sx_de_args *a, int finalize, void *stream) {
    if (int rc = check_args(a)) return rc;
    Enqueue q((hipStream_t)stream);
    return enqueue_de_generation(q, a, finalize);
}

// hipGraph of ngen generations: 2*ngen kernel nodes in a chain (4*ngen for rows of more than kMaxDim elements)
extern "C" int sx_de_graph_create(const sx_de_args *a, int ngen, sx_graph **out) {
    if (int rc = check_args(a)) return rc;
    SX_REQUIRE(out != nullptr && ngen >= 1 && a->gbest != nullptr, "sx_de_graph_create: bad arguments");
    SX_REQUIRE(a->rng == SX_RNG_PHILOX, "sx_de_graph_create: graphs need in-kernel (Philox) draws");
    GraphBuild gb;
    if (int rc = gb.begin()) return rc;
    for (int i = 0; i < ngen; ++i)
        if (int rc = enqueue_de_generation(gb.sink(), a, 1)) return rc;
    return gb.finish(out);
}

// Multi-GPU: this shard's generation + its best-of-generation record, one host call (the caller then
// all-gathers the records and calls sx_gather_finalize).
extern "C" int sx_de_shard_generation(const sx_de_args *a, double *record, void *stream) {
    SX_REQUIRE(record != nullptr, "sx_de_shard_generation: null record");
    if (int rc = sx_de_generation(a, 0, stream)) return rc;
    return sx_shard_best(a->part_f, a->part_i, (int64_t)geometry(a).blocks, a->buf0, a->buf1, a->ld, a->n, a->state,
                         a->row0, record, stream);
}

// ---------------------------------------------------------------------------
// Chained finalize (single GPU, Philox): one kernel per generation.
// ---------------------------------------------------------------------------
// every wavefront of the single-GPU chained kernel re-reduces the workgroup records, so only while those are
// few; in the peer-exchange kernel only the service workgroup reads them (any number)
static int check_chain(const sx_de_args *a, bool peer_exchange) {
    if (int rc = check_args(a)) return rc;
    SX_REQUIRE(a->rng == SX_RNG_PHILOX, "sx_de_chain: needs in-kernel (Philox) draws");
    SX_REQUIRE(!is_wide(a->n, de_wide_from(a)), "sx_de_chain: rows served by the one-workgroup-per-row kernels (n > wide_from) take the two-kernel path (sx_de_generation)");
    SX_REQUIRE(peer_exchange || geometry(a).blocks <= 512,
               "sx_de_chain: more than 512 workgroup records (use the two-kernel path)");
    return 0;
}

// x == nullptr: single GPU (XM = 1); otherwise the peer-exchange kernel (XM = 2, one service workgroup in front)
static int enqueue_de_chain(Enqueue &q, const sx_de_args *a, const sx_xchg_args *x, int parity, int finalize_only) {
    PlanArg plan;
    if (make_plan_arg(a->fun_id, a->n, &plan)) return -1;
    const Geometry g = geometry(a);
    const de_kernel_t kern = x ? de_p2p_kernel(a->fun_id, a->n, a->P, a->strategy, a->constraints)
                               : de_chain_kernel(a->fun_id, a->n, a->P, a->strategy, a->constraints);
    const unsigned blocks = finalize_only ? 1u : g.blocks + (x ? 1u : 0u);
    const int64_t npart = g.blocks;
    // (the four leading arguments are scalars of their own: the single-GPU kernel has them preloaded, sx_de_kernel.hpp)
    return q.kernel(kern, dim3(blocks), dim3(g.threads), g.lds, a->state + parity, a->part_f + parity * npart,
                    a->part_i + parity * npart, npart, *a, plan, parity, finalize_only ? 1 : 0, x ? *x : sx_xchg_args{});
}

static int chain_launch(const sx_de_args *a, const sx_xchg_args *x, int parity, int finalize_only, void *stream) {
    if (int rc = check_chain(a, x != nullptr)) return rc;
    SX_REQUIRE(parity == 0 || parity == 1, "sx_de_chain_launch: parity must be 0 or 1");
    Enqueue q((hipStream_t)stream);
    return enqueue_de_chain(q, a, x, parity, finalize_only);
}

static int chain_graph_create(const sx_de_args *a, const sx_xchg_args *x, int ngen, int start_parity, sx_graph **out) {
    if (int rc = check_chain(a, x != nullptr)) return rc;
    SX_REQUIRE(out != nullptr && ngen >= 1 && (start_parity == 0 || start_parity == 1),
               "sx_de_chain_graph_create: bad arguments");
    GraphBuild gb;
    if (int rc = gb.begin()) return rc;
    for (int i = 0; i < ngen; ++i)
        if (int rc = enqueue_de_chain(gb.sink(), a, x, (start_parity + i) & 1, 0)) return rc;
    return gb.finish(out);
}

extern "C" int sx_de_chain_launch(const sx_de_args *a, int parity, int finalize_only, void *stream) {
    return chain_launch(a, nullptr, parity, finalize_only, stream);
}
extern "C" int sx_de_chain_graph_create(const sx_de_args *a, int ngen, int start_parity, sx_graph **out) {
    return chain_graph_create(a, nullptr, ngen, start_parity, out);
}

// ---------------------------------------------------------------------------
// Multi-GPU, peer exchange: the chained kernel on this rank's shard (a->P rows from global row a->row0)
// ---------------------------------------------------------------------------
extern "C" int sx_de_p2p_launch(const sx_de_args *a, const sx_xchg_args *x, int parity, int finalize_only,
                                void *stream) {
    if (int rc = check_xchg_args(x)) return rc;
    return chain_launch(a, x, parity, finalize_only, stream);
}
extern "C" int sx_de_p2p_graph_create(const sx_de_args *a, const sx_xchg_args *x, int ngen, int start_parity,
                                      sx_graph **out) {
    if (int rc = check_xchg_args(x)) return rc;
    return chain_graph_create(a, x, ngen, start_parity, out);
}

extern "C" int sx_graph_launch(sx_graph *g, void *stream) {
    SX_REQUIRE(g && g->exec, "sx_graph_launch: null graph");
    SX_HIP(hipGraphLaunch(g->exec, (hipStream_t)stream));
    return 0;
}

extern "C" int sx_graph_destroy(sx_graph *g) {
    if (!g) return 0;
    if (g->exec) (void)hipGraphExecDestroy(g->exec);
    if (g->graph) (void)hipGraphDestroy(g->graph);
    if (g->scratch) (void)hipFree(g->scratch);
    delete g;
    return 0;
}
