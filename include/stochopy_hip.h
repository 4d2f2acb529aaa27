/*
 * stochopy_hip.h -- C ABI of the MI355X (gfx950) population-evaluation engine.
 *
 * Drop-in boundary for the per-generation hot path of keurfonluu/stochopy v2.3.0
 * (a pure-Python/numpy package: there is no FFI in the reference; these are the
 * entry points a `backend="hip"` branch of its backend hook would bind through
 * ctypes -- see INTEGRATION.md).  Each entry point cites the reference code it
 * replaces (paths relative to the reference checkout).
 *
 * Conventions
 *   - plain pointers and sizes only; no torch / numpy types.
 *   - every `double*` / `int*` marked DEVICE points into HBM owned by the caller;
 *     the library never allocates or frees caller memory.
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream).
 *     All kernels are asynchronous on that stream.
 *   - return value: 0 = ok, negative = error (text via sx_last_error()).
 *   - float64 throughout, as in the reference; compiled
 *     with -ffp-contract=off so a*b+c rounds twice like numpy does.
 *   - populations are row-major (P, ld) with ld >= n (row stride in doubles).
 */
#ifndef STOCHOPY_HIP_H
#define STOCHOPY_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SX_ABI_VERSION 1

/* objective ids: stochopy/factory/benchmark.py:14-156 */
enum {
    SX_FUN_ACKLEY = 0,          /* benchmark.py:14-34   */
    SX_FUN_GRIEWANK = 1,        /* benchmark.py:37-56   */
    SX_FUN_QUARTIC = 2,         /* benchmark.py:59-76   */
    SX_FUN_RASTRIGIN = 3,       /* benchmark.py:79-97   */
    SX_FUN_ROSENBROCK = 4,      /* benchmark.py:100-118 */
    SX_FUN_SPHERE = 5,          /* benchmark.py:121-136 */
    SX_FUN_STYBLINSKI_TANG = 6, /* benchmark.py:139-156 */
    SX_FUN_COUNT = 7
};

/* DE strategies: stochopy/optimize/de/_strategy.py:1-46 */
enum { SX_DE_RAND1BIN = 0, SX_DE_RAND2BIN = 1, SX_DE_BEST1BIN = 2, SX_DE_BEST2BIN = 3 };

/* random-draw source for the generation kernels */
enum {
    SX_RNG_HOST = 0,   /* draws uploaded by the host (numpy-legacy MT19937 stream, parity mode) */
    SX_RNG_PHILOX = 1  /* Philox4x32-10 generated in-kernel, counter = (slot,row,gen,purpose)    */
};

/* termination status, stochopy/optimize/_common.py:13-24 */
#define SX_STATUS_NONE 100

int sx_abi_version(void);
const char *sx_last_error(void);
/* number of visible HIP devices (<0 on error); used by the loader to fail loudly */
int sx_device_count(void);
/* sizeof(sx_state / sx_de_args / sx_pso_args / sx_xchg_args) as compiled: lets a binding check its struct
 * mirror (which: 0 state, 1 DE args, 2 PSO args, 3 exchange args, 4 CMA state, 5 CMA args, 6 VD-CMA args, 7 sampler args,
 * 8 DE-runs args, 9 PSO-runs args, 10 CMA-runs args, 12 row-wise runs args; -1 otherwise, 11 included: the VD-CMA runs'
 * struct is checked through sx_vd_runs_args_bytes) */
int sx_struct_size(int which);

/* ------------------------------------------------------------------------- *
 * Summation plan: numpy's pairwise add.reduce order for a length-m vector
 * (numpy/_core/src/umath/loops_utils.h.src, blocksize 128).
 * The objective kernels follow it so fitness values are bit-identical to the
 * reference's `.sum()` for +,-,* objectives.  Host function, exported so tests can
 * pin the order; the kernels receive the plan in their arguments (scalar loads),
 * built by the library from (fun_id, n).
 *   out[0]=nleaf out[1]=tail out[2]=full 8-blocks out[3]=stack depth
 *   out[4+2t]=end block of leaf t, out[5+2t]=merges after leaf t
 * Returns the number of int32 written (<= cap), or <0 if cap is too small.
 * ------------------------------------------------------------------------- */
int sx_sum_plan(int64_t m, int32_t *out, int cap);
/* number of terms the objective sums for an n-vector (n or n-1) */
int64_t sx_fun_terms(int fun_id, int n);

/* ------------------------------------------------------------------------- *
 * Batched objective evaluation  f[i] = fun(X[i,:])
 * replaces: the population wrapper stochopy/optimize/_common.py:34-90
 *           (serial :79-80, joblib :39-43, MPI :58-72) applied to the
 *           benchmark objectives, and cmaes/_cmaes.py:167-173 when xm/xstd are
 *           given (x -> x*xstd + xm before the objective).
 * X DEVICE (P,ldx); f DEVICE (P); xm/xstd DEVICE (n) or NULL.
 * part_f/part_i DEVICE (sx_num_partials(P,n)) or NULL: per-workgroup (min f, first row)
 * records for sx_select_finalize.  16, 32 or 64 lanes evaluate one individual; n <= 4096.
 * ------------------------------------------------------------------------- */
int64_t sx_num_partials(int64_t P, int n);
int sx_rows_per_workgroup(int n); /* rows of one workgroup of the row kernels = rows behind one (part_f, part_i) record */
/* Rows of more than this many elements are served by the one-workgroup-per-row kernels (one record per row, no chained /
 * peer-exchange form): what a host loop needs to know to size its record buffers and to pick the two-kernel path.  2048:
 * where the one-workgroup-per-row kernels become the faster ones. */
int sx_wide_from(void);
/* sx_num_partials for a DE run whose sx_de_args.wide_from is `wide_from` (0: sx_wide_from()). */
int64_t sx_de_num_partials(int64_t P, int n, int wide_from);
int sx_eval(int fun_id, const double *X, int64_t P, int n, int64_t ldx, const double *xm, const double *xstd,
            double *f, double *part_f, int64_t *part_i, void *stream);

/* Initial population with in-kernel draws (rng="philox"): the Latin hypercube of
 * _common.py:109-120 (strata of width 2/P, jitter of width 1/P, one stratum per row and column, scaled to the
 * bounds with the reference's two-rounding arithmetic), every row computable on its own: stratum = keyed bijection
 * of [0, P) per column (Philox keys), jitter = 53-bit Philox uniform keyed by (global row, element).  A rank of a
 * sharded run draws only its rows [row0, row0 + rows) of the P-row population.  X DEVICE (rows, ld); lower/upper
 * DEVICE (n).  Oracle counterpart: oracle/streams.py PhiloxStream.lhs_population. */
int sx_philox_lhs(double *X, int64_t rows, int n, int64_t ld, int64_t row0, int64_t P, const double *lower,
                  const double *upper, uint32_t key0, uint32_t key1, void *stream);

/* argmin with numpy's first-minimum tie rule (np.argmin, _common.py:132, de/_de.py:216)
 * f DEVICE (P); ws_f/ws_i DEVICE scratch of ws_len >= 1 entries; out_idx/out_val DEVICE (1). */
int sx_argmin(const double *f, int64_t P, double *ws_f, int64_t *ws_i, int64_t ws_len, int64_t *out_idx,
              double *out_val, void *stream);

/* ------------------------------------------------------------------------- *
 * Generation state shared by DE and PSO (64 bytes, DEVICE; host reads it back)
 * ------------------------------------------------------------------------- */
typedef struct sx_state {
    int64_t it;      /* generations completed (the reference's `it`; initial evaluation = 1) */
    int64_t gbidx;   /* row of the current best                                             */
    double gfit;     /* best fitness                                                         */
    double dx;       /* ||xbest_prev - xbest|| of the last selection (_common.py:135)        */
    int32_t status;  /* SX_STATUS_NONE while running, else -1 / 0 / 1 (_common.py:134-158)   */
    int32_t done;    /* 1 once status is set: later generation launches are no-ops           */
    int64_t reserved[3];
} sx_state;

/* ------------------------------------------------------------------------- *
 * Differential Evolution, synchronous generation
 * replaces: de/_de.py:314-351 de_sync (mutation via _strategy.py, binomial
 *           crossover `r1 <= CR` + forced index, de/_constraints.py:13-28 Random)
 *           + _common.py:123-160 selection_sync + the objective calls, fused.
 * Population storage: two row buffers buf0/buf1 (P,ld); generation g (= state->it)
 * lives in buf[g & 1].  A generation reads X_i and its k donor rows from the
 * current buffer and writes row i of the other one (the trial vector if it wins
 * with strict <, else the unchanged row), so donor reads never race with
 * selection writes and a generation moves (k+2) rows per individual
 * (SURVEY.md section 8d).
 * ------------------------------------------------------------------------- */
typedef struct sx_de_args {
    double *buf0, *buf1;    /* DEVICE (P,ld) each                                     */
    double *fit;            /* DEVICE (P) personal-best fitness (pbestfit)            */
    double *candfit;        /* DEVICE (P) candidate fitness `pfit` or NULL            */
    double *gbest;          /* DEVICE (n) copy of the best row (maintained by sx_select_finalize);
                               NULL = read row state->gbidx of the current buffer       */
    const double *lower;    /* DEVICE (n)                                             */
    const double *upper;    /* DEVICE (n)                                             */
    sx_state *state;        /* DEVICE                                                 */
    double *part_f;         /* DEVICE (sx_de_num_partials(P, n, wide_from))           */
    int64_t *part_i;        /* DEVICE (sx_de_num_partials(P, n, wide_from))           */
    /* SX_RNG_HOST inputs for ONE generation (the numpy-legacy stream, App. B):      */
    const double *r1;       /* DEVICE (P,n) rand(P,n), de/_de.py:250                  */
    const int32_t *donors;  /* DEVICE (k,P) first k rows of delete_shuffle_sync, :304 */
    const int32_t *irand;   /* DEVICE (P) randint(n,size=P), :340                     */
    const double *resample; /* DEVICE (P,n) uniform(lo,hi,(P,n)) or NULL, _constraints.py:24 */
    int64_t P;
    int64_t ld;
    int64_t row0;           /* global index of local row 0 (Philox counters; multi-GPU shards) */
    int32_t n;
    int32_t fun_id;
    int32_t strategy;
    int32_t constraints;    /* 0 none, 1 Random                                       */
    int32_t rng;            /* SX_RNG_HOST / SX_RNG_PHILOX                            */
    int32_t maxiter;
    int32_t wide_from;      /* rows of more than this many elements take the one-workgroup-per-row kernels; 0 = sx_wide_from().
                               Clamped to [256, 4096], the rows the wavefront-per-row kernels can serve.  A run that needs the
                               chained kernel's peer exchange or global-donor gathers on rows of 2049 ... 4096 elements sets 4096 */
    int32_t spec_store;     /* single-GPU chained kernel, rows of up to 128 elements: when a row is stored.  0 = the trial
                               before the objective and the row that won again after it (what runs), 1 = once, after the
                               objective; 2 / 3 (measurement aids) = the trial / the old row before the objective and
                               afterwards only the rows for which that was the wrong one.  Same results whichever it is; the
                               other kernels ignore it (this word was padding: size and layout of the struct are unchanged) */
    double F, CR, xtol, ftol;
    uint32_t key0, key1;    /* Philox key = seed                                      */
} sx_de_args;

/* one generation: propose+evaluate+select kernel, then (if finalize) the
 * best/termination kernel.  finalize=0 is for multi-GPU, where the caller
 * exchanges the shard bests first and then calls sx_select_finalize itself. */
int sx_de_generation(const sx_de_args *a, int finalize, void *stream);

/* ------------------------------------------------------------------------- *
 * Best-of-generation + termination: _common.py:131-158 (argmin, xtol/ftol/maxiter ladder)
 * Reduces the per-workgroup partials, computes dx against `gbest`, sets status,
 * copies the new best row into `gbest`, increments state->it.
 * The best row is read from rows[(state->it+1) & 1] (the generation being
 * finalised; pass rows0 == rows1 for state that is updated in place, e.g. PSO pbest).
 * Rows of more than 4096 elements (three launches: the best record, the row's slices on up to 64 workgroups, the state):
 * the records are CONSUMED -- the first min(npart, 64) doubles of part_f are reused for the slices' partial squared
 * distances, so part_f holds no records afterwards (it is declared const for the common case; read the records, if
 * wanted, before this call).
 * ------------------------------------------------------------------------- */
int sx_select_finalize(const double *part_f, const int64_t *part_i, int64_t npart, const double *rows0,
                       const double *rows1, int64_t ld, int n, double *gbest, sx_state *state, int maxiter,
                       double xtol, double ftol, void *stream);

/* ------------------------------------------------------------------------- *
 * Multi-GPU (population sharded by rows, one process per GPU): the per-generation exchange that
 * takes the place of the reference's MPI Bcast/Allreduce (stochopy/optimize/_common.py:58-72).
 * sx_shard_best: this shard's best of the generation being finalised ->
 *     record (n+2 doubles) = [ f, (double)(row0 + local row), row[0..n) ]
 * The caller all-gathers the records of all ranks (RCCL over xGMI) into `records` (world,(n+2)).
 * sx_gather_finalize: first minimum over the records by (f, global row) = np.argmin over the whole
 *     population, then the same dx / status / gbest / state update as sx_select_finalize.
 * ------------------------------------------------------------------------- */
int sx_shard_best(const double *part_f, const int64_t *part_i, int64_t npart, const double *rows0,
                  const double *rows1, int64_t ld, int n, const sx_state *state, int64_t row0, double *record,
                  void *stream);
int sx_gather_finalize(const double *records, int world, int n, double *gbest, sx_state *state, int maxiter,
                       double xtol, double ftol, void *stream);
/* sx_de_generation(a, 0) + sx_shard_best in one host call (fewer launches' worth of host time per generation) */
int sx_de_shard_generation(const struct sx_de_args *a, double *record, void *stream);

/* ------------------------------------------------------------------------- *
 * hipGraph of `ngen` identical generations (all per-generation state lives in
 * `state` on the device, so one instantiated graph is replayed).
 * Only valid for SX_RNG_PHILOX (host draws change every generation).
 * ------------------------------------------------------------------------- */
typedef struct sx_graph sx_graph;
int sx_de_graph_create(const sx_de_args *a, int ngen, sx_graph **out);
/* Chained finalize (single GPU, SX_RNG_PHILOX): ONE kernel per generation.  a->state must point to
 * sx_state[3] and a->part_f / a->part_i to [2][sx_num_partials(P,n)].  Launch L uses parity L & 1: every
 * workgroup first re-reduces the records its predecessor wrote to part[parity] (the best-of-generation /
 * termination step of _common.py:131-158, published in state[1-parity] by workgroup 0) and then produces
 * the next generation with records in part[1-parity].  finalize_only: just that first half, result in
 * state[2] (what the host reads).  The kernel stops on fun <= ftol with status 1; status 0 (xtol) is settled
 * by the caller from state.reserved[0] = the previous best row.  Start: state[0] = {it 0, gbidx}, part[0] =
 * {(f_best, row_best), +inf...}, generation 1 in buf1. */
int sx_de_chain_launch(const sx_de_args *a, int parity, int finalize_only, void *stream);
int sx_de_chain_graph_create(const sx_de_args *a, int ngen, int start_parity, sx_graph **out);
int sx_graph_launch(sx_graph *g, void *stream);
int sx_graph_destroy(sx_graph *g);

/* ------------------------------------------------------------------------- *
 * Multi-GPU, peer exchange over xGMI (one process per GPU; population sharded by rows)
 * replaces: the per-generation MPI traffic of stochopy/optimize/_common.py:58-72 (Bcast + Allreduce)
 *           for the global best of _common.py:131-133.
 * Every rank owns an exchange buffer in its HBM (uncached, IPC-shareable) that all peers map.  It holds
 * slots[2][world][2*(n+2)] 64-bit words: the record [f, global row, best row] of each rank, each 32-bit
 * half carried with a 32-bit generation tag in one 8-byte store (arrival is detected on the data itself,
 * no separate flag, no fence).  sx_de_p2p_* = the chained kernel of sx_de_chain_* where, per generation,
 * workgroup 0 writes this shard's record straight into every peer's slot and every wavefront picks the
 * global best out of its own rank's slots as they arrive: still ONE kernel per generation and no
 * collective call on the data path.  A rank that waits longer than `timeout_ticks` (100 MHz ticks) sets
 * *error and the kernels become no-ops (the caller raises).
 * Start as for sx_de_chain_launch with a->gbest = NULL; afterwards the best row of the last generation is
 * slot[parity][state.reserved[1]] (decode with sx_xchg_read_record), the previous one is in the other parity.
 * ------------------------------------------------------------------------- */
#define SX_MAX_PEERS 8
#define SX_IPC_HANDLE_BYTES 64
typedef struct sx_xchg_args {
    uint64_t *peer[SX_MAX_PEERS]; /* DEVICE: exchange buffer of rank r as mapped in this process (peer[rank] = own) */
    int32_t world, rank;
    int64_t timeout_ticks;        /* per wait, in 100 MHz ticks (1e8 = 1 s) */
    int32_t *error;               /* DEVICE: 0, set to 1 on timeout */
    uint64_t *relay;              /* DEVICE, ordinary (cacheable) memory, sx_xchg_relay_bytes(n), zeroed: rows of
                                     more than 128 elements are read from here after workgroup 0 has copied the
                                     winning record out of the uncached exchange buffer (once per generation,
                                     instead of once per wavefront) */
    /* donors over the WHOLE population (exact reference semantics, de/_de.py:304-311, at the price of remote
     * row reads over xGMI): global_rows = world * shard_rows > 0 and pop0/pop1[r] = rank r's two population
     * buffers (sx_pop_alloc + sx_xchg_open).  global_rows = 0: donors are drawn inside the shard. */
    const double *pop0[SX_MAX_PEERS];
    const double *pop1[SX_MAX_PEERS];
    int64_t global_rows, shard_rows;
} sx_xchg_args;
/* bytes of one exchange buffer for `world` ranks and rows of n doubles (includes the probe area) */
int64_t sx_xchg_bytes(int world, int n);
int64_t sx_xchg_relay_bytes(int n);
/* allocate + zero an exchange buffer on the current device and export it (handle: 64 bytes) */
int sx_xchg_alloc(int64_t bytes, void **ptr, void *handle);
int sx_xchg_free(void *ptr);
/* ordinary device memory that peers can map (population buffers read remotely with global donors); release with
 * sx_xchg_free, map / unmap with sx_xchg_open / sx_xchg_close */
int sx_pop_alloc(int64_t bytes, void **ptr, void *handle);
/* map a peer's buffer from the handle it exported / unmap it */
int sx_xchg_open(const void *handle, void **ptr);
int sx_xchg_close(void *ptr);
/* transport self-test: `rounds` tagged all-to-all writes + waits through the probe area of the buffers;
 * returns 0 = every word of every round arrived, 1 = timeout or corrupt word (synchronises the stream) */
int sx_xchg_probe(const sx_xchg_args *x, int n, int rounds, void *stream);
/* decode slot[parity][src] of the own buffer into record[n+2] (host memory); synchronises the stream */
int sx_xchg_read_record(const sx_xchg_args *x, int n, int parity, int src, double *record, void *stream);
/* The same exchange as ONE one-workgroup kernel for generation kernels that are not chained (PSO / CPSO):
 * sx_shard_best + all-gather + sx_gather_finalize without a collective -- shard best from the workgroup
 * records, record into every peer's slot, wait for all ranks, global best, dx, gbest, status, it++
 * (_common.py:131-158).  rows0/rows1, ld, row0 as for sx_shard_best; gbest/state as for sx_gather_finalize. */
int sx_xchg_finalize(const double *part_f, const int64_t *part_i, int64_t npart, const double *rows0,
                     const double *rows1, int64_t ld, int n, int64_t row0, double *gbest, sx_state *state, int maxiter,
                     double xtol, double ftol, const sx_xchg_args *x, void *stream);
int sx_de_p2p_launch(const sx_de_args *a, const sx_xchg_args *x, int parity, int finalize_only, void *stream);
int sx_de_p2p_graph_create(const sx_de_args *a, const sx_xchg_args *x, int ngen, int start_parity, sx_graph **out);

/* ------------------------------------------------------------------------- *
 * PSO / CPSO, synchronous generation
 * replaces: cpso/_cpso.py:324-329 mutation (V = w*V + c1*r1*(pbest-X) + c2*r2*(gbest-X),
 *           left-to-right), cpso/_constraints.py:4-10 / 44-53 (X+V, or Shrink: per-row
 *           beta = min over violated dims of (bound-x)/v), cpso/_cpso.py:332-361 pso_sync
 *           + _common.py:123-160 selection_sync (cand = X, x = pbest) + the objective.
 * X, V, pbest, pbestfit are updated in place (row-local state).
 * ------------------------------------------------------------------------- */
typedef struct sx_pso_args {
    double *X, *V, *pbest;  /* DEVICE (P,ld) each                                     */
    double *pbestfit;       /* DEVICE (P)                                             */
    double *candfit;        /* DEVICE (P) fitness of the new positions `pfit`, or NULL */
    double *gbest;          /* DEVICE (n) copy of the best row (sx_select_finalize)   */
    const double *lower;    /* DEVICE (n)                                             */
    const double *upper;    /* DEVICE (n)                                             */
    sx_state *state;        /* DEVICE                                                 */
    double *part_f;         /* DEVICE (sx_num_partials(P,n))                          */
    int64_t *part_i;        /* DEVICE (sx_num_partials(P,n))                          */
    const double *r1;       /* DEVICE (P,n) rand(P,n), cpso/_cpso.py:262  (SX_RNG_HOST) */
    const double *r2;       /* DEVICE (P,n) rand(P,n), cpso/_cpso.py:263  (SX_RNG_HOST) */
    const uint64_t *pending_restart; /* DEVICE (3) or NULL: an sx_pso_restart_select decision (its out3) of the
                             * PREVIOUS generation that sx_pso_restart_apply has not carried out: the generation kernel
                             * re-seeds those rows itself (same Philox positions, V = 0, pbest = X, pbestfit = 1e30,
                             * cpso/_cpso.py:420-424) instead of loading them.  Set inside sx_pso_graph_create only
                             * (in-kernel draws); callers pass NULL and apply restarts with sx_pso_restart_apply. */
    int64_t P;
    int64_t ld;
    int64_t row0;           /* global index of local row 0 (Philox counters; shards)  */
    int32_t n;
    int32_t fun_id;
    int32_t constraints;    /* 0 none, 1 Shrink                                       */
    int32_t rng;
    int32_t maxiter;
    int32_t pad_;
    double w, c1, c2, xtol, ftol;
    uint32_t key0, key1;
} sx_pso_args;

int sx_pso_generation(const sx_pso_args *a, int finalize, void *stream);

/* Competitive restart, cpso/_cpso.py:405-426.
 * sx_pso_radius: part_r[b] = max over the rows of workgroup b of ||X_i - gbest||_2 (:410)
 *   part_r DEVICE (sx_num_partials(P,n)).
 * sx_pso_restart_select (one workgroup; keys in registers up to 32768 particles, re-read from L2 above): radius = max(part_r)/sqrt(4n); if
 *   radius < delta: nw = int((P-1)/(1+exp((it/maxiter-gamma+0.5)/0.09))) and the nw-th largest
 *   pbestfit (radix descent).  out3 DEVICE uint64[3] = {nw, threshold key, radius bits}.
 * sx_pso_restart_apply: rows with pbestfit among the nw worst get V=0, X=uniform(lower,upper),
 *   pbest=X, pbestfit=1e30 (:420-424).  Either sel3 (device selection, Philox positions keyed
 *   by row) or host_rows/host_x (DEVICE copies of the reference-ordered row ids and their
 *   numpy-legacy positions, host_count rows). */
int sx_pso_radius(const sx_pso_args *a, double *part_r, void *stream);
int sx_pso_restart_select(const sx_pso_args *a, const double *part_r, double delta, double gamma, uint64_t *out3,
                          void *stream);
int sx_pso_restart_apply(const sx_pso_args *a, const uint64_t *sel3, const int64_t *host_rows, const double *host_x,
                         int64_t host_count, void *stream);
/* Sharded swarm (one process per GPU, a->P rows each): the same selection over the WHOLE swarm.
 * gathered DEVICE (world, a->P + sx_num_partials(a->P, n)): row r = rank r's [pbestfit | part_r] after one
 * all-gather per generation (the allreduce(max) of the radius and the fitness all-gather of SURVEY.md
 * section 8e in one message).  Every rank computes the same {nw, threshold, radius}. */
int sx_pso_restart_select_gathered(const sx_pso_args *a, const double *gathered, int world, double delta,
                                   double gamma, uint64_t *out3, void *stream);
/* hipGraph of `ngen` generations of the cpso loop body (cpso/_cpso.py:257-307), single GPU + SX_RNG_PHILOX:
 * per generation sx_pso_generation(a, 1) and, when part_r/sel3 are given (CPSO), the radius and selection kernels; a
 * decided restart is carried out by the next generation's kernel (sx_pso_args.pending_restart, set here), the apply
 * kernel runs once after the last generation, so X / V / pbest are complete whenever a replay has finished.
 * Replay with sx_graph_launch; launches after convergence are no-ops. */
int sx_pso_graph_create(const sx_pso_args *a, int ngen, double *part_r, double delta, double gamma, uint64_t *sel3,
                        sx_graph **out);

/* ------------------------------------------------------------------------- *
 * Generations around a CALLER-SUPPLIED objective (the backend hook contract of _common.py:27-106: `fun(X)` maps
 * the (P,n) population to (P,) values -- here a callable working on the device array).  The objective cannot
 * be fused, so a generation is: sx_de_propose / sx_pso_move -> caller's objective -> sx_rows_select ->
 * sx_select_finalize (or the shard-best exchange).  Same draws / arithmetic / records as the fused kernels.
 *   sx_de_propose : cand (P,n) row-major <- the trial vectors of generation state->it + 1 (de/_de.py:333-344,
 *                   de/_strategy.py, de/_constraints.py:13-28); nothing else is written.
 *   sx_pso_move   : V, X updated in place (cpso/_cpso.py:324-329, cpso/_constraints.py:4-53).
 *   sx_rows_select: selection_sync after the evaluation (_common.py:127-129): rows with f[i] < xfun[i] take
 *                   cand[i] (xout row <- cand row, xfun[i] <- f[i]); the others keep xin's row (copied when
 *                   xout != xin: DE's other population buffer); candfit[i] <- f[i] (or NULL); part_f/part_i <-
 *                   the workgroup records sx_select_finalize / sx_shard_best expect. */
int sx_de_propose(const sx_de_args *a, double *cand, void *stream);
int sx_pso_move(const sx_pso_args *a, void *stream);
int sx_rows_select(const double *cand, int64_t ldc, const double *f, const double *xin, double *xout, int64_t ldx,
                   double *xfun, double *candfit, int64_t P, int n, const sx_state *state, double *part_f,
                   int64_t *part_i, void *stream);

/* ------------------------------------------------------------------------- *
 * updating="immediate": ONE asynchronous generation, i.e. the ordered sweep in which individual i sees
 * what individuals 0..i-1 did in the same generation (csrc/sx_async.hip: one workgroup; rounds of up to 64
 * individuals are proposed together, judged in order, and the few that depended on an earlier one of their
 * round are proposed again -- the sequential result, bit for bit).
 * replaces: de/_de.py:354-391 de_async, cpso/_cpso.py:364-402 pso_async, _common.py:163-194 selection_async
 *           (`<=` acceptance, best row + status updated per individual, the last individual's status wins,
 *           then `it >= maxiter -> -1`), cpso/_constraints.py:56-64 (Shrink, one-row form), objective fused.
 * State: population in place (DE: a->buf0 only; PSO: X, V, pbest), a->gbest (n) in/out = the best row,
 * a->state->it / gfit in/out, status / done out.  SX_RNG_HOST inputs as for the synchronous generation, but
 * drawn in the asynchronous order (sx_mt_de_async_draws).  part_f / part_i / buf1 are not used.
 * Single GPU (row0 = 0, P = whole population). */
int sx_de_async_generation(const sx_de_args *a, void *stream);
int sx_pso_async_generation(const sx_pso_args *a, void *stream);

/* ------------------------------------------------------------------------- *
 * CMA-ES device kernels (fp64 MFMA, v_mfma_f64_16x16x4_f64, LDS-tiled 64x64x32)
 * sx_cmaes_sample   replaces cmaes/_cmaes.py:232-237:
 *     arx[i,:] = xmean + sigma * dot(B, D * Z[i,:])          Z (P,n) standard normals
 * sx_cmaes_recombine replaces cmaes/_cmaes.py:274:
 *     xmean = dot(w, arx[idx[:mu], :])                        idx DEVICE int64 (mu), best first
 * sx_cmaes_rank_mu  replaces cmaes/_cmaes.py:290-295 (in place on C, full matrix as the reference):
 *     artmp = (arx[idx[:mu]] - xold) / sigma
 *     C = C*(1-c1-cmu) + cmu * artmp^T diag(w) artmp + c1 * outer(pc,pc) + tmp_coef * C_old
 *     with tmp_coef = 0 when `cond` holds, else c1*cc*(2-cc)  (:291)
 * sx_cmaes_normals  in-kernel Philox Box-Muller normals (throughput mode of :234)
 * sx_symmetrize_upper replaces cmaes/_cmaes.py:303: C = triu(C) + triu(C,1).T
 * All pointers DEVICE.  The eigendecomposition (:304, numpy/LAPACK in the reference) and the
 * scalar path/step-size/convergence logic stay on the host.
 * ------------------------------------------------------------------------- */
int sx_cmaes_sample(const double *xmean, double sigma, const double *B, const double *D, const double *Z, double *arx,
                    int64_t P, int n, void *stream);
int sx_cmaes_recombine(const double *arx, const int64_t *idx, const double *w, int mu, int n, double *xmean,
                       void *stream);
int sx_cmaes_rank_mu(const double *arx, const int64_t *idx, const double *w, int mu, const double *xold, double sigma,
                     const double *pc, double c1, double cmu, double tmp_coef, double *C, double *ws_y, int n,
                     void *stream); /* ws_y: DEVICE scratch (mu,n) for artmp */
int sx_cmaes_normals(double *Z, int64_t P, int n, int64_t row0, uint32_t gen, uint32_t key0, uint32_t key1,
                     void *stream);
int sx_symmetrize_upper(double *C, int n, void *stream);
/* CMA-ES box-constraint handling "Penalize", device part.
 * replaces: cmaes/_constraints.py:29-31 (candidates clipped to the standardised box [-1,1]^n, then the objective)
 *           and :79 (arfitness += dot((arxvalid - arx)**2, bnd_weights / bnd_scale)); the scalar bookkeeping
 *           of :33-76 (percentiles, weight history) stays on the host as in the reference.
 * X DEVICE (P,n) standardised candidates; xm/xstd DEVICE (n); v DEVICE (n) = bnd_weights / bnd_scale or NULL;
 * f_raw DEVICE (P) = fun(unstandardise(clip(X))); pen DEVICE (P) = sum_j (clip(x_ij) - x_ij)^2 v_j (NULL with v). */
int sx_cmaes_eval_penalized(int fun_id, const double *X, int64_t P, int n, const double *xm, const double *xstd,
                            const double *v, double *f_raw, double *pen, void *stream);
/* VD-CMA sampling, vdcma/_vdcma.py:236-248: for candidates row0 .. row0+P-1 of the generation
 *   ary[i] = dvec o (Z[i] + coef * (Z[i] . vn) * vn)   (coef = sqrt(1 + |v|^2) - 1),   arx[i] = xmean + sigma * ary[i];
 * dy != NULL: global rows 0 and 1 become +dy / -dy (mean-shift injection, :241-247).
 * Z, ary, arx DEVICE (P,n); dvec, vn, xmean, dy DEVICE (n).  One wavefront per candidate, O(n). */
int sx_vdcma_sample(const double *Z, int64_t P, int n, int64_t row0, const double *dvec, const double *vn, double coef,
                    const double *xmean, double sigma, const double *dy, double *ary, double *arx, void *stream);

/* ------------------------------------------------------------------------- *
 * CMA-ES, device-resident generation (csrc/sx_cma_loop.hip): one call enqueues a whole generation --
 * normals, sampling (MFMA), objective, ranking, recombination, evolution paths, step size, covariance
 * update (MFMA), [symmetrise + sx_eigh], the ten stopping rules -- and the host looks at the 128-byte
 * state only every few generations.
 * replaces cmaes/_cmaes.py:226-343 (one pass of the `while` loop) and :360-434 (`converge`), for draws made on the
 * device (Philox), constraints=None, one GPU.  Everything in sx_cma_args is DEVICE memory unless stated.
 *   gen       1-based generation number (the caller counts; it also keys the Philox normals)
 *   do_eigh   the caller's evaluation of :301 (`nfev - eigeneval > popsize / (c1 + cmu) / ndim / 10`, a function of
 *             gen only): 0 not due, 1 decompose, 2 decompose starting from the previous eigenvectors in B
 * After a stopping rule has fired (state->done) the bookkeeping kernels of later calls do nothing and
 * xbest / state keep the result; besthist must be zero-initialised (the reference's np.zeros(maxiter), :220).
 * ------------------------------------------------------------------------- */
typedef struct sx_cma_state {
    int64_t it;         /* generations completed                                                       */
    int64_t nfev;       /* it * popsize                                                                */
    int64_t best_row;   /* arindex[0] of the last generation                                           */
    double fbest;       /* arfitness[arindex[0]]                                                       */
    double sigma;       /* step size entering the next generation                                      */
    double sigma_next;  /* scratch: step size after :298, published by the stop step                   */
    double tmp_coef;    /* 0 when `cond` held (:283-291), else c1*cc*(2-cc)                            */
    double psnorm;      /* |ps|                                                                        */
    int32_t status;     /* SX_STATUS_NONE while running, else the reference's status (-8 .. 1)         */
    int32_t done;       /* 1 once a stopping rule fired                                                */
    int64_t stop_it;    /* generation at which it fired                                                */
    double reserved[6]; /* [0..4] VD-CMA's model scalars; [5] arfitness.argmin() of the last generation    */
} sx_cma_state;

typedef struct sx_cma_args {
    double *Z, *arx;            /* (P,n) normals / candidates (standardised coordinates)              */
    double *fit;                /* (P)                                                                */
    double *xmean, *xold, *ps, *pc; /* (n)                                                            */
    double *C, *B;              /* (n,n) covariance, eigenvectors in columns                          */
    double *D;                  /* (n) sqrt of the eigenvalues                                        */
    double *eigw;               /* (n) eigenvalues as sx_eigh returns them                            */
    const double *w;            /* (mu) recombination weights                                         */
    double *Y;                  /* (mu,n) scratch of the covariance update                            */
    double *part;               /* (64,n) scratch of the recombination                                */
    double *step, *isc, *xnew;  /* (n) scratch: xmean - xold, C^(-1/2) step, the new mean             */
    double *ypart;              /* (8,n) scratch of B^T step                                          */
    double *besthist;           /* (maxiter) zero-initialised                                         */
    const double *xm, *xstd;    /* (n) un-standardisation x * xstd + xm (:167-173)                    */
    double *xbest;              /* (n) result: best candidate of the stopping generation              */
    double *hist_x, *hist_f;    /* return_all history (maxiter, rows, n) / (maxiter, rows), un-standardised candidates
                                 * (:262-269), or NULL; rows = hist_rows, or 1 when hist_rows == 0 (best candidate only) */
    int64_t *order;             /* (P) argsort of fit                                                 */
    void *state;                /* sx_cma_state                                                       */
    void *eigh_ws;              /* sx_eigh workspace                                                  */
    double *pen_ws;             /* constraints="Penalize" on the device (cmaes/_constraints.py:4-82), or NULL: doubles
                                 * [weights n | v n | penalty P | spread history 256 | count, validfitval, iniphase, -];
                                 * initialise weights = 0, history[0] = 1, count = 1, validfitval = 0, iniphase = 1.  Needs
                                 * int(20 + 3n/P) + 1 <= 256 history entries (else: the host-driven loop)   */
    int64_t *pen_order;         /* (P) argsort of the raw fitness (percentiles of :34-35), with pen_ws      */
    int64_t eigh_ws_bytes;
    int64_t P;
    int64_t hist_rows;          /* ceil(verbosity * popsize)                                          */
    int32_t n, mu, fun_id, maxiter, ilim, eig_sweeps;
    double cs, cc, c1, cmu, damps, chind, mueff, xtol, ftol, insigma;
    uint32_t key0, key1;
} sx_cma_args;

int sx_cmaes_generation(const sx_cma_args *a, int64_t gen, int do_eigh, void *stream);
/* The ranking step of the device-resident CMA-ES / VD-CMA generations on its own: order = np.argsort(fit, kind="stable")
 * (NaN last, ties by lower index); with besthist, state (an sx_cma_state) gets best_row / fbest = order[0] and
 * reserved[5] = np.argmin(fit) (the first NaN if any), besthist[gen - 1] = fit[order[0]].  Nothing happens once state.done. */
int sx_cma_rank(const double *fit, int64_t P, int64_t *order, void *state, double *besthist, int64_t gen, void *stream);
/* The Penalize step of the device-resident CMA-ES / VD-CMA generations on its own (cmaes/_constraints.py:4-82): pen_order =
 * argsort of the fit GIVEN (the percentiles are taken of it), the boundary-weight bookkeeping in pen_ws, then fit = objective
 * of the clipped arx + the weighted squared excess (pen_ws's penalty slots).  Reads of h: arx, fit, xm, xstd, xmean, xold,
 * state (its sigma and done), pen_ws, pen_order, n, P, mueff, fun_id, and C (its diagonal) when dvec == NULL; dvec / vvec
 * DEVICE (n): the diagonal is d (1 + v^2) d (VD-CMA).  Non-zero, nothing launched: a null pointer among those, a bad shape,
 * or a spread history of more than 256 entries (20 + 3n/P + 1 > 256).  Once state.done the ranking, the bookkeeping and the
 * addition rest (pen_ws's weights, v, history and flags keep their values); the evaluation still writes fit. */
int sx_cma_penalize(const sx_cma_args *h, int64_t gen, const double *dvec, const double *vvec, void *stream);
/* The same generation in two steps for candidates sharded over ranks (workers > 1; what the reference's parallel backends
 * shard: _common.py:58-72).  stage 0: this rank's candidates [row0, row0 + rows) -- Philox normals keyed by the global
 * row, sampling GEMM, objective -- into arx_loc (rows,n) / fit_loc (rows); the caller
 * all-gathers them into a->arx / a->fit; stage 1: everything else (ranking ... stop rules; Penalize's bookkeeping and
 * penalty pass), replicated on every rank.  stage 0 with all rows + stage 1 == sx_cmaes_generation.
 * a->Z must be the struct's full (P, n) buffer on EVERY rank, not a per-shard one: stage 0 uses its first rows x n doubles
 * for the normals, and stage 1's covariance update takes 2 n n doubles of it as split-K scratch whenever P >= 2 n (always
 * inside the (P, n) buffer then; with P < 2 n the update runs unsplit and needs none). */
int sx_cmaes_generation_stage(const sx_cma_args *a, int64_t gen, int do_eigh, int stage, int64_t row0, int64_t rows,
                              double *arx_loc, double *fit_loc, void *stream);
/* The generation with its decomposition (cmaes/_cmaes.py:301-309; do_eigh != 0) enqueued in pieces, one GPU: phase 0 =
 * candidates + model update up to and including the decomposition's start and its rounds [0, r1); the caller reads the
 * eigensolver's run record (the head of a->eigh_ws: int32 done_seq, sweeps, parity, converged; sx_eigh_info) and either adds
 * rounds (phase 1: [r0, r1)) or lets phase 2 (r1 = rounds enqueued so far) finish the decomposition and apply the stop rules.
 * Same kernels in the same order as sx_cmaes_generation, minus the no-op launches behind the run's end (a sweep's worth per
 * decomposition when the allowance has to be guessed in advance).  sx_eigh_rounds_per_sweep(n): rounds of one sweep of the
 * block method; 0 for the one-workgroup solver of small n, which cannot be enqueued in pieces. */
int sx_eigh_rounds_per_sweep(int n);
int sx_cmaes_generation_phased(const sx_cma_args *a, int64_t gen, int do_eigh, int phase, int r0, int r1, void *stream);

/* ------------------------------------------------------------------------- *
 * Symmetric eigendecomposition on the device (csrc/sx_eigh.hip): parallel two-sided block Jacobi, the
 * similarity updates as fp64 MFMA tile products, convergence decided on the device.
 * replaces cmaes/_cmaes.py:303-305:
 *     C = triu(C) + triu(C,1).T;  D, B = np.linalg.eigh(C);  idx = argsort(D);  D = D[idx];  B = B[:, idx]
 * (numpy.linalg.eigh = LAPACK dsyevd, the reference's third-party call).
 * C DEVICE (n,n) row-major, only its upper triangle is read (mirrored, as :303 does); w DEVICE (n) eigenvalues
 * ascending; B DEVICE (n,n) row-major, eigenvector k in column k, unit norm, CANONICAL SIGN: the component of
 * largest magnitude (lowest row on ties) is positive.  V0: NULL, or DEVICE (n,n) nearly orthonormal starting basis
 * (e.g. the eigenvectors of the previous, slightly different matrix; may alias B): it is re-orthonormalised (one
 * Newton-Schulz step) and the iteration starts from V0^T C V0 -- same result to rounding, fewer sweeps; ignored for
 * n <= 32 (one-workgroup path).  ws: DEVICE scratch of
 * sx_eigh_workspace_bytes(n) bytes; it starts with the run record read by sx_eigh_info.  max_sweeps <= 0: 24;
 * tol <= 0: 1e-14 (a sweep is the last one when the off-diagonal mass it leaves behind -- measured on the device
 * while its last rotations are applied -- is <= tol*|C|_F).
 * Asynchronous on `stream`; the host never waits: launches after convergence are no-ops.
 * sx_eigh_info (synchronises): sweeps carried out, whether the rule was met, off-diagonal mass / |C|_F left
 * behind by the last sweep.
 * The refinement step: the last sweep of a run may be replaced by the first-order refinement step
 * V <- V (I + K + K K / 2), K_ij = M_ij / (M_jj - M_ii), once what the sweeps left is small against every gap
 * (off(M) <= 1e-7 |C|_F and max |K_ij| <= 1e-3, both measured on the device; csrc/sx_eigh.hip kRefineOff).
 * It is allowed inside the CMA-ES generation loops (sx_cmaes_generation*) and not in sx_eigh itself; the environment
 * variable SX_EIGH_REFINE = 0 / 1, read once, forbids / allows it in both.  sx_eigh_refined decides it per call.
 * (Removed after commit c68e4cc: the process-wide setters sx_eigh_set_refine / sx_eigh_set_flow, and with the latter the
 * resident one-launch form of the rounds -- bit-identical to the launch per round and no faster, profiles/r6_eigh_flow.txt.)
 * ------------------------------------------------------------------------- */
int64_t sx_eigh_workspace_bytes(int n);
int sx_eigh(const double *C, int n, const double *V0, double *w, double *B, void *ws, int64_t ws_bytes, int max_sweeps,
            double tol, void *stream);
/* sx_eigh with the refinement step allowed (refine > 0) / forbidden (0) for THIS call (< 0: the library's default, as sx_eigh) */
int sx_eigh_refined(const double *C, int n, const double *V0, double *w, double *B, void *ws, int64_t ws_bytes,
                    int max_sweeps, double tol, int refine, void *stream);
int sx_eigh_info(const void *ws, int *sweeps, int *converged, double *off_rel, void *stream);

/* VD-CMA: everything of the model update that is O(mu n), on the device.
 * replaces vdcma/_vdcma.py:289-295 (w . arx[arindex[:mu]]), :317 (w . ary[arindex[:mu]]) and :331-339 with :428-444 (the
 * weighted moments p, q of the selected steps under D (I + v v^T) D):
 *   out[0*n ..] = sum_k w_k arx[idx_k]        out[1*n ..] = sum_k w_k ary[idx_k]
 *   out[2*n ..] = p_mu                        out[3*n ..] = q_mu                 (y_k = ary[idx_k] / dvec, t_k = y_k . vn)
 * arx, ary DEVICE (P,n); idx DEVICE int64 (mu) best first; w, dvec, vn DEVICE; ws DEVICE scratch of
 * (mu rounded up to 8) + 4*64*n doubles; out DEVICE (4,n).  The host keeps the O(n) natural-gradient step. */
int sx_vdcma_moments(const double *arx, const double *ary, const int64_t *idx, const double *w, int mu, int n,
                     const double *dvec, const double *vn, double norm_v2, double *ws, double *out, void *stream);

/* VD-CMA, device-resident generation (csrc/sx_cma_loop.hip): the whole loop body of vdcma/_vdcma.py:232-425 between two
 * looks of the host at the state -- normals, the mean-shift injection (:241-247), candidates, objective, ranking, the
 * O(mu n) moment sums, and in ONE workgroup the O(n) part: mean / step (:292-295), the rank-gap step size (:298-306),
 * the evolution path (:309-314), alpha / beta (:317-328), the moments of the path, the natural gradient and the update
 * of v and d (:331-378), the stopping rules (cmaes/_cmaes.py:360-434 without the rules that need B, D).
 * state: an sx_cma_state whose reserved[0..4] = {ps, |v|^2, |v|, injection flag, sqrt(1 + |v|^2) - 1}; sigma_next,
 * tmp_coef, psnorm unused.  All vectors DEVICE; besthist zero-initialised; hist_x / hist_f as in sx_cma_args or NULL. */
typedef struct sx_vd_args {
    double *Z, *ary, *arx;      /* (P,n) normals / steps y / candidates x.  Wide models (n > 4096) without hist_x and pen_ws:
                                 * arx may be NULL -- x = xmean + sigma y is then not kept (a quarter of a generation's memory
                                 * traffic): the moment sums and the result form it again from y, same bits.  Wide models use
                                 * Z for t_k (P doubles) and eight words behind them only.                                    */
    double *fit;                /* (P)                                                                */
    double *xmean, *xold, *dx, *dvec, *vvec, *vn, *pc; /* (n)                                         */
    double *zinj, *dy;          /* (n) the injection's normal row ("row P" of the generation) and +-dy */
    const double *w;            /* (mu)                                                               */
    double *mws, *mout;         /* sx_vdcma_moments' workspace and its (4,n) output                    */
    double *besthist;           /* (maxiter)                                                          */
    const double *xm, *xstd;    /* (n) un-standardisation                                             */
    double *xbest;              /* (n) result                                                         */
    double *hist_x, *hist_f;    /* return_all history slabs or NULL                                   */
    int64_t *order;             /* (P) argsort of the generation's fitness                             */
    void *state;                /* sx_cma_state                                                       */
    double *pen_ws;             /* constraints="Penalize" on the device, or NULL: as sx_cma_args.pen_ws (the covariance
                                 * diagonal is that of D (I + v v^T) D, vdcma/_vdcma.py:249-254)        */
    int64_t *pen_order;         /* (P), with pen_ws                                                   */
    int64_t P;
    int64_t hist_rows;
    int32_t n, mu, fun_id, maxiter, ilim, pad_;
    double cs, ds, cc, c1, cmu, mueff, wsum, xtol, ftol, insigma;
    uint32_t key0, key1;
} sx_vd_args;

int sx_vdcma_generation(const sx_vd_args *a, int64_t gen, void *stream);
/* two steps around one all-gather for candidates sharded over ranks, as sx_cmaes_generation_stage (stage 0 fills
 * ary_loc / arx_loc (rows,n) and fit_loc (rows) for rows [row0, row0 + rows); the injected pair is global rows 0, 1).
 * Stage 1 of a generation follows stage 0 of the SAME generation on the same stream: for wide models stage 0 also zeroes the
 * barrier words (behind t_k in Z) of the one-launch model update that stage 1 enqueues. */
int sx_vdcma_generation_stage(const sx_vd_args *a, int64_t gen, int stage, int64_t row0, int64_t rows, double *ary_loc,
                              double *arx_loc, double *fit_loc, void *stream);

/* ------------------------------------------------------------------------- *
 * Neighbourhood Algorithm: the resampling walk (csrc/sx_na.hip)
 * replaces na/_na.py:265-305 mutation(), everything that is O(popsize * models * ndim):
 *   sx_na_begin    X[i] = model kidx[i];  d2[i][m] = ((U[:, 1:] - X[i, 1:]) ** 2).sum(axis=1)  (:277-280, numpy's
 *                  pairwise order) for every stored model m
 *   sx_na_axis     axis step j of all walks: the pending `d2 += (U[:, jp] - X[i, jp]) ** 2 - (U[:, jp+1] - X[i, jp+1]) ** 2`
 *                  of the previous free axis jp (-1: none), lim (:288), low / high (:290-294),
 *                  X[i, j] = low + (high - low) * u[i, j] (:296: np.random.uniform(low, high)); xnew[i] = X[i, j]
 *   sx_na_commit   fixed axes of the finished samples -> 0 (:283-286) and the samples appended to the model store
 *   sx_na_uniforms the generation's uniforms from the device generator (Philox, rng="philox")
 * The scalar recurrence d1 (:298-300: numpy SCALAR `** 2` = libm pow) is evaluated by the caller between two
 * axis steps and handed in as d1[i].  Models are stored column-major: XT[l * cap + m]; kidx DEVICE int64 (P) store
 * positions; X DEVICE (P,n) the samples being built; d2 DEVICE (P,cap); u DEVICE (P,n) doubles in [0,1);
 * ws DEVICE scratch of 2 * P * sx_na_blocks(M) doubles; fixed DEVICE int32 (n), 1 where upper == lower.
 * ------------------------------------------------------------------------- */
int sx_na_blocks(int64_t M);
int sx_na_begin(const double *XT, int64_t cap, int64_t M, int n, const int64_t *kidx, int64_t P, double *X, double *d2,
                void *stream);
int sx_na_axis(const double *XT, int64_t cap, int64_t M, int n, int j, int jp, const int64_t *kidx, int64_t P,
               const double *u, const double *d1, double *X, double *d2, double *ws, double *xnew, void *stream);
int sx_na_commit(double *X, int64_t P, int n, const int32_t *fixed, double *XT, int64_t cap, int64_t M, void *stream);
int sx_na_uniforms(double *U, int64_t P, int n, uint32_t gen, uint32_t key0, uint32_t key1, void *stream);

/* ------------------------------------------------------------------------- *
 * numpy-legacy random stream (host): bit-exact MT19937 replica of what the
 * reference draws through np.random.* after np.random.seed(seed)
 * (de/_de.py:148-149, cpso/_cpso.py:153-154, cmaes/_cmaes.py:116-117;
 * algorithms: SURVEY.md Appendix A).  Host memory only.
 * ------------------------------------------------------------------------- */
typedef struct sx_mt sx_mt;
sx_mt *sx_mt_create(uint32_t seed);                       /* np.random.seed(seed)                 */
void sx_mt_destroy(sx_mt *g);
void sx_mt_seed(sx_mt *g, uint32_t seed);
void sx_mt_random(sx_mt *g, double *out, int64_t count);  /* rand / uniform(size=)               */
void sx_mt_uniform(sx_mt *g, double lo, double hi, double *out, int64_t count); /* uniform(lo,hi,size) */
void sx_mt_uniform_rows(sx_mt *g, const double *lo, const double *hi, int n, int64_t rows,
                        double *out);                     /* uniform(lo[n],hi[n],(rows,n))       */
void sx_mt_randn(sx_mt *g, double *out, int64_t count);   /* randn / normal(0,1) (polar, cached) */
void sx_mt_randint(sx_mt *g, int64_t high, int64_t *out, int64_t count); /* randint(high,size=)  */
void sx_mt_permutation(sx_mt *g, int64_t n, int64_t *out); /* permutation(n)                     */
/* _common.py:109-120 lhs: rand(P,n) then n x permutation(P); out[i][j] = (x[perm_j[i]][j]) * scale[j] + shift[j] with
 * x = rand / P + lin[i]; lin (P) = numpy's linspace(-1, 1, P, endpoint=False), scale / shift (n) = 0.5*(upper -/+ lower) */
void sx_mt_latin_hypercube(sx_mt *g, int64_t P, int n, const double *lin, const double *scale, const double *shift,
                           double *out);
/* de/_de.py:304-311 delete_shuffle_sync: P permutations of P-1, first k rows kept: donors[k][P] */
void sx_mt_de_donors(sx_mt *g, int64_t P, int k, int32_t *donors);
/* the per-individual draws of ONE de_async generation after r1 (de/_de.py:376-382): for i = 0..P-1
 * permutation(delete(arange(P), i)) -> donors[t*P+i] (t < k), randint(n) -> irand[i], and with
 * constraints="Random" uniform(lower, upper, n) -> resample[i*n ..] (resample NULL: not drawn) */
void sx_mt_de_async_draws(sx_mt *g, int64_t P, int k, int n, int32_t *donors, int32_t *irand, const double *lower,
                          const double *upper, double *resample);
/* interchange with np.random.get_state()/set_state(): key[624], pos, has_gauss, cached_gaussian */
void sx_mt_get_state(sx_mt *g, uint32_t *key, int *pos, int *has_gauss, double *gauss);
void sx_mt_set_state(sx_mt *g, const uint32_t *key, int pos, int has_gauss, double gauss);

/* ------------------------------------------------------------------------- *
 * Samplers: many independent, device-resident Markov chains (csrc/sx_sample.hip).
 * Replaces the sample loops of stochopy/sample/mcmc/_mcmc.py:104-156 (Metropolis-Hastings, one block of
 * k = max(1, int(perc * ndim)) variables perturbed per sample) and stochopy/sample/hmc/_hmc.py:135-185 with
 * numerical_gradient (:215-231): one row group per chain, the chain's rows in LDS for the whole launch, no
 * exchange between chains.  One launch advances every chain by `steps` samples.
 *
 * Draws: rng = SX_RNG_HOST reads them from `normals` / `logu` (one chain: the reference's own stream, drawn by
 * the host in the reference's order); SX_RNG_PHILOX makes them in the kernel, counter = (slot, chain, sample,
 * purpose) -- a chain's draws depend on its index and the key only.
 *
 * Per-chain state (all DEVICE, written by the launch that generates sample 0 and carried from launch to launch):
 *   cur (C,n) current sample, fcur (C) its value, nacc (C) accepted proposals, nfeas (C) proposals that passed the
 *   feasibility test, facc / iacc (C) best ACCEPTED value and its sample index (inf / 0 while nothing was accepted:
 *   the reference's fmin / imin), fmin / imin (C) numpy's argmin over the samples so far (first NaN wins),
 *   xbest (C,n) the sample the method reports as x: iacc's for mcmc, imin's for hmc.
 * ------------------------------------------------------------------------- */
enum { SX_SAMPLE_MCMC = 0, SX_SAMPLE_HMC = 1, SX_SAMPLE_ENSEMBLE = 2 /* the sx_sample_ensemble_* entry points only */ };
enum { SX_JAC_FINITE_DIFF = 0, SX_JAC_ANALYTIC = 1 };

typedef struct sx_sample_args {
    double *cur, *fcur, *facc, *fmin, *xbest;
    int64_t *iacc, *imin, *nacc, *nfeas;
    const double *x0;      /* initial samples, row stride x0_stride (0: one row for all chains); NULL: Philox uniform in the box */
    double *xall, *funall; /* (C, maxiter, n) / (C, maxiter), or both NULL (return_all off) */
    const double *lower, *upper, *step; /* (n); step = stepsize * 0.5 * (upper - lower), formed by the caller */
    const double *normals; /* SX_RNG_HOST: mcmc (maxiter-1, k) block normals of samples 1.., hmc (maxiter-1, n) momenta */
    const double *logu;    /* SX_RNG_HOST: (maxiter) log of the acceptance uniform of sample i (entry 0 unused) */
    int64_t C, x0_stride, maxiter;
    int32_t n, fun_id, method, rng, reject /* constraints="Reject" */, k /* mcmc block length */, nleap, jac;
    double fd_step;        /* hmc finite_diff_abs_step */
    uint32_t key0, key1;
} sx_sample_args;

/* samples [it0, it0 + steps) of every chain; it0 = 0 starts the chains (sample 0 is the initial point) */
int sx_sample_run(const sx_sample_args *a, int64_t it0, int64_t steps, void *stream);
/* chains one workgroup carries for this method / row length (launch geometry; results do not depend on it) */
int sx_sample_chains_per_workgroup(int method, int jac, int n);
/* G[i,:] = analytic gradient of objective fun_id at X[i,:] (the hmc kernel's device functions), X / G (P,n) DEVICE */
int sx_sample_gradient(int fun_id, const double *X, int64_t P, int n, double *G, void *stream);

/* ------------------------------------------------------------------------- *
 * Samplers around a CALLER-SUPPLIED objective (csrc/sx_sample_unfused.hip): the objective (and, for hmc, the gradient)
 * is evaluated between the launches below, on (C, n) device arrays.  Same draws, arithmetic and per-chain state as
 * sx_sample_run: with bit-identical objective / gradient values the run is sx_sample_run's, bit for bit.  rng must be
 * SX_RNG_PHILOX; fun_id, normals and logu are not read.  Every function is one launch; prop / pmom / q / G are (C, n)
 * DEVICE, fprop / k0 (C) DEVICE.
 *   sample `it` of mcmc:  propose -> fprop = fun(prop) -> decide
 *   sample `it` of hmc:   propose -> (nleap + 2) x (G = gradient(prop) -> leap) -> fprop = fun(prop) -> decide
 *   sample 0:             propose -> fprop = fun(prop) -> decide
 * ------------------------------------------------------------------------- */
/* replaces mcmc/_mcmc.py:93 and hmc/_hmc.py:124 (it = 0: prop = the initial point), mcmc/_mcmc.py:106-118 (prop = cur with
 * block (it-1) mod ceil(n/k) perturbed) and hmc/_hmc.py:137-141 (prop = cur, pmom = randn(n), k0 = 0.5 sum pmom^2).
 * pmom / k0 may be NULL for mcmc */
int sx_sample_propose(const sx_sample_args *a, int64_t it, double *prop, double *pmom, double *k0, void *stream);
/* replaces hmc/_hmc.py:143-155, one step: pmom -= (coef * step) * G; then, if move, q += step * pmom
 * (coef = 0.5 for the first and the last of the nleap + 2 momentum steps, move = 0 for the last) */
int sx_sample_leap(const sx_sample_args *a, double coef, int move, double *q, double *pmom, const double *G, void *stream);
/* replaces the rows numerical_gradient evaluates (hmc/_hmc.py:217-233), axes [axis0, axis0 + naxes) of every chain:
 * W (naxes, 2, C, n) DEVICE, W[i,0,c,:] = q[c,:] with component axis0+i moved by +fd_step, W[i,1,c,:] by -fd_step, the
 * components before it carrying the reference's in-place round trip ((q + h) - h, (q - h) + h) */
int sx_sample_fd_rows(const sx_sample_args *a, const double *q, int axis0, int naxes, double *W, void *stream);
/* replaces hmc/_hmc.py:227-233: fW (naxes, 2, C) DEVICE the objective's values of those rows ->
 * G[c, axis0+i] = (0.5 * (fW[i,0,c] - fW[i,1,c])) / fd_step */
int sx_sample_fd_gradient(const sx_sample_args *a, const double *fW, int axis0, int naxes, double *G, void *stream);
/* replaces mcmc/_mcmc.py:120-140 and hmc/_hmc.py:157-172: feasibility (reject), the acceptance draw and decision with
 * fprop = fun(prop), the chain's counts and best samples, row `it` of xall / funall (it = 0 starts the chains: cur = prop).
 * pmom / k0 (hmc: what propose and the leaps left) may be NULL for mcmc */
int sx_sample_decide(const sx_sample_args *a, int64_t it, const double *prop, const double *fprop, const double *pmom,
                     const double *k0, void *stream);

/* ------------------------------------------------------------------------- *
 * Per-chain step-size adaptation in a warm-up, and recording with a burn-in and thinning.  No counterpart in the
 * reference.  sx_sample_args stays what it is; the options travel in a second struct, and the *_adapt entry points take the
 * arguments of sx_sample_run / _propose / _leap / _decide with it behind `a`.  rng must be SX_RNG_PHILOX.
 *
 * Chain c carries a multiplier s_c (1.0 at the start): wherever a sample reads step[e] it reads s_c * step[e], formed first
 * (mcmc: v + z * (s step[e]); hmc: p - (coef * (s step[e])) * g and q + (s step[e]) * p); with s = 1.0 that is
 * sx_sample_run's arithmetic bit for bit.  After the decision of sample `it`, 1 <= it <= warmup, with t = (double)it and d the
 * sample's own d (mcmc fcur - fprop, hmc U0 - U + K0 - K) -- dual averaging (Hoffman & Gelman 2014):
 *     alpha   = infeasible (reject) ? 0 : d < 0 ? exp(d) : d >= 0 ? 1 : 0       (a NaN d counts as 0 HERE; it still accepts)
 *     eta     = 1 / (t + 10);   hbar = (1 - eta) * hbar + eta * (target - alpha)
 *     logs    = log(10) - (sqrt(t) / 0.05) * hbar
 *     w       = 1 / (sqrt(t) * sqrt(sqrt(t)))
 *     logsbar = w * logs + (1 - w) * logsbar
 *     s       = it < warmup ? exp(logs) : exp(logsbar)                          (frozen from sample warmup + 1 on)
 * and at it == warmup nacc is copied to nacc_warm.  The accept / reject decision is not changed.
 * Recording: sample `it` goes to row (it - rec_start) / rec_every of xall (C, rec_rows, n) / funall (C, rec_rows) when
 * it >= rec_start and (it - rec_start) % rec_every == 0; rec_rows = ceil((maxiter - rec_start) / rec_every).
 * With warmup = 0, rec_start = 0, rec_every = 1 every output is sx_sample_run's, bit for bit.
 * ------------------------------------------------------------------------- */
typedef struct sx_sample_adapt {
    double *scale, *hbar, *logsbar; /* DEVICE (C): s_c and the two averages; written by the launch that generates sample 0 */
    int64_t *nacc_warm;             /* DEVICE (C): nacc after sample `warmup`.  All four may be NULL when warmup == 0 */
    int64_t warmup;                 /* 0 <= warmup <= maxiter - 1 */
    int64_t rec_start, rec_every;   /* 0 <= rec_start <= maxiter - 1, 1 <= rec_every < 2^31 */
    int64_t rec_rows;               /* rows of xall / funall per chain */
    double target;                  /* the acceptance the rule steers to, in (0, 1) (read when warmup > 0) */
} sx_sample_adapt;
/* sizeof(sx_sample_adapt) as the library was built (sx_struct_size is not extended) */
int sx_sample_adapt_bytes(void);
int sx_sample_run_adapt(const sx_sample_args *a, const sx_sample_adapt *ad, int64_t it0, int64_t steps, void *stream);
int sx_sample_propose_adapt(const sx_sample_args *a, const sx_sample_adapt *ad, int64_t it, double *prop, double *pmom,
                            double *k0, void *stream);
int sx_sample_leap_adapt(const sx_sample_args *a, const sx_sample_adapt *ad, double coef, int move, double *q, double *pmom,
                         const double *G, void *stream);
int sx_sample_decide_adapt(const sx_sample_args *a, const sx_sample_adapt *ad, int64_t it, const double *prop,
                           const double *fprop, const double *pmom, const double *k0, void *stream);

/* ------------------------------------------------------------------------- *
 * Per-axis scale adaptation in the warm-up (a diagonal metric).  No counterpart in the reference.  On top of sx_sample_adapt:
 * chain c carries m_c[e] (1.0 at the start) and eff_c[e] = m_c[e] * step[e]; an adapting sample reads s * eff[e] where it
 * read s * step[e] (the same association), the momenta stay randn(n) and the kinetic energy 0.5 sum p^2 -- leap-frog in
 * coordinates rescaled per axis; the decision is not changed.  The *_metric entry points take the arguments of the *_adapt
 * forms with this struct behind `ad`.
 *
 * Windows: b_0 = win_start < b_1 = win_end[0] < ... < b_J = win_end[nwin - 1] <= warmup.  After the decision of sample `it`
 * with b_{j-1} < it <= b_j, x the chain's current state and N = it - b_{j-1}, per element (Welford):
 *     delta = x - mean;  mean += delta / N;  M2 += delta * (x - mean)
 * At it == b_j, after that and after the sample's step of the dual averaging, with h_e = 0.5 * (upper_e - lower_e):
 *     var = M2 / (N - 1);   v = (N / (N + 5)) * var + ((5 / (N + 5)) * 1e-3) * (h_e * h_e);   r_e = sqrt(v)
 *     L = (sum_e log r_e) / n;   m_e = r_e / exp(L);   eff_e = m_e * step[e]
 * unless some r_e is not finite or not positive: the chain then keeps its m.  mean and M2 are zeroed.  Then the step size
 * restarts: sbase <- sbase * exp(logsbar) (1.0 at the start), hbar = logsbar = 0, the multiplier in use is sbase, and the
 * rule's clock is t = (double)(it - b_j) for the samples that follow; while adapting s = sbase * exp(logs), at it == warmup
 * s = sbase * exp(logsbar).  With nwin = 0 every output is the *_adapt form's, bit for bit, and the four pointers may be NULL.
 * ------------------------------------------------------------------------- */
typedef struct sx_sample_metric {
    double *sbase;           /* DEVICE (C): the multiplier the dual averaging restarted from */
    double *m, *mean, *M2;   /* DEVICE (C, n): the scales and the running moments of the open window */
    int32_t nwin;            /* 0 <= nwin <= 8 */
    int64_t win_start;       /* b_0 >= 0 */
    int64_t win_end[8];      /* b_1 < ... < b_nwin <= warmup */
} sx_sample_metric;
/* sizeof(sx_sample_metric) as the library was built (sx_struct_size is not extended) */
int sx_sample_metric_bytes(void);
int sx_sample_run_metric(const sx_sample_args *a, const sx_sample_adapt *ad, const sx_sample_metric *mt, int64_t it0,
                         int64_t steps, void *stream);
int sx_sample_propose_metric(const sx_sample_args *a, const sx_sample_adapt *ad, const sx_sample_metric *mt, int64_t it,
                             double *prop, double *pmom, double *k0, void *stream);
int sx_sample_leap_metric(const sx_sample_args *a, const sx_sample_adapt *ad, const sx_sample_metric *mt, double coef, int move,
                          double *q, double *pmom, const double *G, void *stream);
int sx_sample_decide_metric(const sx_sample_args *a, const sx_sample_adapt *ad, const sx_sample_metric *mt, int64_t it,
                            const double *prop, const double *fprop, const double *pmom, const double *k0, void *stream);

/* ------------------------------------------------------------------------- *
 * Parallel tempering (replica exchange) for the Metropolis-Hastings chains (csrc/sx_sample_temper.hip): C ladders of K
 * device-resident replicas.  No counterpart in the reference.  Replica q = c K + k is rung k of ladder c and samples
 * p^(beta[k]), beta[k] = 1 / T_k with 1 = T_0 < T_1 < ...: sx_sample_run's mcmc sample with d = (fcur - fprop) * beta[k]
 * and every draw keyed by q in the place of the chain index (beta[0] = 1.0: the cold rung's rule is sx_sample_run's,
 * bit for bit).  After sample it >= 1 with it % swap_every == 0 the exchange event j = it / swap_every pairs rungs
 * (0,1), (2,3), ... (odd j) or (1,2), (3,4), ... (even j); a rung without a partner sits out.  The pair (k, k+1)
 * exchanges its STATES (cur and fcur; rungs stay) when  min(0, d) > log(u),  d = (beta[k] - beta[k+1]) (f_k - f_{k+1})
 * (a NaN d exchanges), u = first double of Philox (slot 0, row = replica of rung k, gen = it, purpose 14).  Sample `it`
 * of a replica is its state after the event; an arriving state is compared with facc / iacc / xbest and fmin / imin as
 * an accepted proposal of sample `it` is, and moves neither nacc nor nfeas.
 * One ladder lives inside one workgroup (an exchange is two workgroup barriers and a row copy in LDS): one launch per
 * run, nothing passes between workgroups, a ladder's run does not depend on C or on the launch geometry.
 * ------------------------------------------------------------------------- */
/* a->C = C*K replicas (every per-chain array that long); a->xall / funall: (C, maxiter, n) / (C, maxiter), cold rungs only;
   beta (K) DEVICE; nswap (C*K) DEVICE int64: accepted exchanges of the pair whose LOWER rung this replica is, carried across
   launches (written by the launch that generates sample 0).  method = SX_SAMPLE_MCMC, rng = SX_RNG_PHILOX. */
int sx_sample_tempered_run(const sx_sample_args *a, const double *beta, int K, int64_t swap_every, int64_t *nswap,
                           int64_t it0, int64_t steps, void *stream);
/* the largest K of a row length: K rows of the mcmc kernel's LDS fit the 160 KiB of a workgroup and its row limit
 * (16 rows, 8 wavefronts); -1 for a row length the samplers do not serve */
int sx_sample_tempered_max_rungs(int n);
/* Around a caller-supplied objective (csrc/sx_sample_unfused.hip), sample `it` of a tempered run:
 *   sx_sample_propose -> fprop = fun(prop) -> sx_sample_decide_tempered -> on an event: sx_sample_swap
 * With bit-identical objective values this is sx_sample_tempered_run's run, bit for bit.
 * sx_sample_decide_tempered: sx_sample_decide for mcmc with beta (K) DEVICE; cold rungs write row `it` of xall / funall at
 * their ladder's index when record != 0 -- pass record = 0 when an odd event follows (sx_sample_swap then writes it). */
int sx_sample_decide_tempered(const sx_sample_args *a, int64_t it, const double *prop, const double *fprop,
                              const double *beta, int K, int record, void *stream);
/* exchange event j (= it / swap_every >= 1) after sample `it`: one row group per pair, the states in device memory (cur,
 * fcur and the best values of a->..., nswap as above).  At odd j it writes row `it` of xall / funall (the state of rung 0
 * after the event).  No launch when no rung has a partner (K = 2, even j). */
int sx_sample_swap(const sx_sample_args *a, int64_t it, int64_t j, const double *beta, int K, int64_t *nswap, void *stream);

/* ------------------------------------------------------------------------- *
 * The affine-invariant ensemble sampler (Goodman & Weare 2010: the stretch move; csrc/sx_sample_ensemble.hip): C ensembles
 * of W device-resident walkers.  No counterpart in the reference.  No step size, no gradient: a walker moves along the line
 * through itself and a walker of the other half of its ensemble, so the sampler performs alike on p(x) and p(Ax + b).
 * W is even, W >= 4 and W >= 2 n; h = W / 2.  Walker w of ensemble g is replica q = g W + w, which takes the chain index's
 * place in every draw and in the per-chain arrays (a->C = C*W, every one that long; a->method = SX_SAMPLE_ENSEMBLE,
 * a->rng = SX_RNG_PHILOX; step, k, nleap, jac, fd_step, normals and logu are not read; x0 is NULL or one row per replica).
 * Sample 0 is the initial state.  Sample it >= 1 is two half-sweeps: half 0 proposes the walkers [0, h) against the walkers
 * [h, W), half 1 the walkers [h, W) against [0, h) as half 0 left them.  The active walker q, with (d0, d1) the two doubles of
 * Philox (slot 0, row q, gen it, purpose 15), base the first walker of the other half and a = stretch:
 *     j = base + min(h - 1, (int)(d0 * h));   z = ((a - 1) * d1 + 1)^2 / a;   Y[e] = X_j[e] + z * (X_q[e] - X_j[e])
 *     d = (n - 1) * log(z) + (fcur_q - f(Y));   accepted when  min(0, d) > log(u)   (a NaN d accepts)
 * u the acceptance draw of (q, it) (purpose 12); with reject a Y outside [lower, upper] is rejected without that draw and
 * nfeas counts the others.  facc / iacc / fmin / imin / xbest follow the mcmc rule per walker.
 * xall (C, maxiter, W, n) / funall (C, maxiter, W): row ((g maxiter + it) W + w).
 * ------------------------------------------------------------------------- */
/* samples [it0, it0 + steps) of every ensemble in ONE launch, one workgroup per ensemble, the walkers in its LDS; it0 = 0
 * starts them.  A run cut into launches is the same run, bit for bit.  Requires 0 < sx_sample_ensemble_lds_bytes(W, n) <=
 * 160 KiB and stretch finite and > 1 */
int sx_sample_ensemble_run(const sx_sample_args *a, int W, double stretch, int64_t it0, int64_t steps, void *stream);
/* HOST only: the dynamic LDS of an ensemble's workgroup, 8 (W n + W + rows (n + 8)) bytes with rows = RPW * min(cap, ceil(h / RPW))
 * row groups, RPW = 4 (n <= 64) or 2 (n <= 128) rows per wavefront and cap = 4 or 8 wavefronts; -1 for a shape the launch does
 * not serve (W odd, < 4 or < 2 n; n < 1 or n > 128) */
int sx_sample_ensemble_lds_bytes(int W, int n);
/* Around a caller-supplied objective, sample 0:  propose(it = 0) -> fprop = fun(prop) on (C*W, n) -> decide(it = 0)
 * and sample it >= 1, for half = 0, 1:           propose -> fprop = fun(prop) on (C*h, n) -> decide
 * Row g h + i of prop / fprop / logzf belongs to walker half * h + i of ensemble g; logzf (C*h) DEVICE takes the factors
 * (n - 1) * log(z) from propose to decide (not used at it = 0, may be NULL there).  The walkers live in a->cur; any n the
 * samplers serve.  With bit-identical objective values this is sx_sample_ensemble_run's run, bit for bit. */
int sx_sample_ensemble_propose(const sx_sample_args *a, int W, double stretch, int64_t it, int half, double *prop,
                               double *logzf, void *stream);
int sx_sample_ensemble_decide(const sx_sample_args *a, int W, int64_t it, int half, const double *prop, const double *fprop,
                              const double *logzf, void *stream);

/* ------------------------------------------------------------------------- *
 * The ensemble sampler with several moves, a burn-in and thinning (csrc/sx_sample_ensemble_moves.hip).  No counterpart in the
 * reference.  The stretch move keeps a walker on the line through itself and one partner, at 1/a to a times their distance
 * from the partner: it cannot carry a walker from one mode of a target into another.  The differential-evolution move (ter
 * Braak 2006) and the snooker move (ter Braak & Vrugt 2008) can.  sx_sample_args stays what it is; the options travel in a
 * second struct, and the *_moves entry points take the arguments of sx_sample_ensemble_run / _propose / _decide with it in
 * the place of `stretch` (decide: behind W).  Everything above holds -- replicas, half-sweeps, the decision, the counters --
 * but the proposal of sample it >= 1:
 *
 * The move.  Ensemble g uses ONE entry k of (kind, cum, param) in both half-sweeps of sample it: with u the first double of
 * Philox (slot 0, row g W, gen it, purpose 16), the first k with cum[k] > u, or nmoves - 1 when there is none (cum: the
 * running sums of the normalised weights, cum[nmoves - 1] = 1.0).
 * SX_ENSEMBLE_STRETCH: the rule above (purpose 15) with a = param[k].
 * The other two draw (d0, d1) from slot 0 and (d2, d3) from slot 1 of Philox (row q, gen it, purpose 17) for the active
 * walker q and pick distinct walkers of the other half, whose first walker is base, by their indices in it:
 *     j1 = min(h - 1, (int)(d0 * h));   j2 = min(h - 2, (int)(d1 * (h - 1)));   j2 += (j2 >= j1)
 * SX_ENSEMBLE_DE, gamma0 = param[k]:
 *     gamma = gamma0 * (1 + 1e-5 * (2 * d2 - 1));   Y[e] = X_q[e] + gamma * (X_j1[e] - X_j2[e]);   d = fcur_q - f(Y)
 * SX_ENSEMBLE_SNOOKER, gammas = param[k] (W >= 6):
 *     j3 = min(h - 3, (int)(d2 * (h - 2)));   j3 += (j3 >= min(j1, j2));   j3 += (j3 >= max(j1, j2))
 *     delta[e] = X_q[e] - X_j1[e];   dd = sum_e delta[e] * delta[e];   pr = sum_e delta[e] * (X_j2[e] - X_j3[e])
 *     c = gammas * (pr / dd), and c = 0 where dd is not > 0 or c is not finite;   Y[e] = X_q[e] + c * delta[e]
 *     d = (n - 1) * log(|1 + c|) + (fcur_q - f(Y))
 * (Y - X_j1 = (1 + c) delta: the factor is |Y - X_j1|^(n-1) / |X_q - X_j1|^(n-1); at c = -1 it is -inf and Y is rejected.)
 * The two sums: lane l of the row's LPR lanes (16 / 32 / 64 for n <= 64 / <= 128 / larger) adds its elements e = l, l + LPR,
 * ... in that order, then v += v[lane ^ 1], ^ 2, ^ 4, ... up to LPR / 2.  No fused multiply-add anywhere.
 *
 * Recording: sample `it` goes to row r = (it - rec_start) / rec_every of xall (C, rec_rows, W, n) / funall (C, rec_rows, W)
 * -- at ((g rec_rows + r) W + w) -- when it >= rec_start and (it - rec_start) % rec_every == 0.  nacc, nfeas and the best
 * values run over all samples.
 * With nmoves = 1, kind[0] = SX_ENSEMBLE_STRETCH, rec_start = 0 and rec_every = 1 every output is that of the entry points
 * above with stretch = param[0], bit for bit.
 * ------------------------------------------------------------------------- */
enum { SX_ENSEMBLE_STRETCH = 0, SX_ENSEMBLE_DE = 1, SX_ENSEMBLE_SNOOKER = 2 };
typedef struct sx_sample_ensemble_opts {
    int32_t nmoves;                 /* 1 <= nmoves <= 4 entries */
    int32_t kind[4];                /* SX_ENSEMBLE_* */
    double cum[4];                  /* 0 < cum[0] < ... < cum[nmoves - 1] = 1.0 */
    double param[4];                /* stretch: a, finite and > 1; de: gamma0, snooker: gammas, finite and > 0 */
    int64_t rec_start, rec_every;   /* 0 <= rec_start <= maxiter - 1, 1 <= rec_every < 2^31 */
    int64_t rec_rows;               /* ceil((maxiter - rec_start) / rec_every): rows of xall / funall per ensemble */
} sx_sample_ensemble_opts;
/* sizeof(sx_sample_ensemble_opts) as the library was built (sx_struct_size is not extended) */
int sx_sample_ensemble_opts_bytes(void);
/* the resident run: one workgroup per ensemble, one launch, the LDS of sx_sample_ensemble_lds_bytes; a run cut into launches
 * is the same run, bit for bit */
int sx_sample_ensemble_run_moves(const sx_sample_args *a, int W, const sx_sample_ensemble_opts *mv, int64_t it0, int64_t steps, void *stream);
/* around a caller-supplied objective, as above; logzf takes the factor 0 / (n - 1) log(z) / (n - 1) log(|1 + c|) to decide.
 * With bit-identical objective values this is sx_sample_ensemble_run_moves's run, bit for bit. */
int sx_sample_ensemble_propose_moves(const sx_sample_args *a, int W, const sx_sample_ensemble_opts *mv, int64_t it, int half, double *prop,
                               double *logzf, void *stream);
int sx_sample_ensemble_decide_moves(const sx_sample_args *a, int W, const sx_sample_ensemble_opts *mv, int64_t it, int half, const double *prop, const double *fprop,
                              const double *logzf, void *stream);

/* ------------------------------------------------------------------------- *
 * Tempered sequential Monte Carlo with evidence (csrc/sx_sample_smc.hip; method="smc").  No counterpart in the reference.
 * C populations of P particles, each independent of the others and of C; particle i of population c is the global row
 * q = c P + i, which keys its draws.  fun = -log likelihood, the prior is uniform on the box: a proposal outside it is always
 * rejected.  The populations go from beta = 0 (the prior) to beta = 1 (the target) and return log Z, Z = the integral of
 * exp(-fun) over the box divided by the box's volume.
 *
 * Stage 0: x_q = initial_value's rule (purpose 13, row q, gen 0), f_q = fun(x_q); beta_0 = 0, logZ = 0, scale_1 = scale.
 * Stage s = 1, 2, ... while beta_{s-1} < 1 and s <= maxiter:
 *  1. fmin = the least finite f.  w_i(beta) = exp(-((beta - beta_{s-1}) * (f_i - fmin))), 0 where f_i is NaN or +inf;
 *     ESS(beta) = (sum w)^2 / sum w^2.  If ESS(1) >= ess * P then beta_s = 1; otherwise lo = beta_{s-1}, hi = 1 and EXACTLY 52
 *     times mid = (lo + hi) / 2; ESS(mid) >= ess * P ? lo = mid : hi = mid; then beta_s = lo > beta_{s-1} ? lo : hi.
 *  2. logZ = logZ + (log(sum w_i(beta_s) / P) - (beta_s - beta_{s-1}) * fmin); reported ESS(beta_s) / P.
 *  3. u = the first double of Philox (slot 0, row c P, gen s, purpose 18); cum the inclusive running sum of w(beta_s) in index
 *     order; ancestor a_i = the least j with cum_j >= ((i + u) / P) * cum_{P-1}, found by bisection (lo = 0, hi = P - 1; mid =
 *     (lo + hi) >> 1; cum_mid >= target ? hi = mid : lo = mid + 1), so P - 1 when there is none.  x_i <- x_{a_i},
 *     f_i <- f_{a_i}, into the other buffer (stage s works in buffer s & 1; stage 0 fills buffer 0).
 *  4. sd_e = the standard deviation (two passes, divisor P) of the resampled population on axis e;
 *     step_e = scale_s * max(sd_e, 1e-8 * h_e), h_e = (upper_e - lower_e) / 2.
 *  5. M = steps Metropolis steps per particle, step m = 1 ... M being sample g = (s - 1) M + m of chain q in the sense of
 *     sx_sample_run: proposal x + step * z on ALL variables (the normals of purpose 10, row q, gen g), feasible when inside
 *     the box, accepted when min(0, d) > log(u'), d = beta_s * (f_cur - f_prop), u' the uniform of purpose 12 (row q, gen g);
 *     a NaN d accepts.
 *  6. r_s = accepted / (P M); scale_{s+1} = scale_s * exp(r_s - target).
 * A population ends after the mutation of the stage with beta_s = 1 (status 0), after maxiter stages with beta < 1 (status -1:
 * its particles sample p^beta), or at the start of a stage where no f is finite or one is -inf (status -2, logZ = -inf).
 * An ended population is frozen: the kernels leave its arrays alone.
 *
 * The order of the sums, fixed by P alone.  Stage kernel (one workgroup of 1 024 threads per population, f in LDS): thread t
 * owns particles [t K, min(P, t K + K)), K = ceil(P / 1024).  sum w and sum w^2: each thread 0.0 + its terms in index order;
 * over the 64 threads of a wave v += v[lane ^ 1], ^ 2, ... ^ 32; then 0.0 + the 16 waves' sums in order.  cum: the threads'
 * totals scanned over the wave (v += v[lane - off] for lane >= off, off = 1, 2, ... 32), base = 0.0 + the totals of the waves
 * before (the wave's last inclusive value), and cum_i = ((base + the exclusive value of the thread) + its own w) + ... one by
 * one.  Gather kernel: for axis e thread r of 16 adds particles r, r + 16, ... in that order from 0.0, the 16 sums are added in
 * the order of r from 0.0; mean = sum / P; the squared deviations from it the same way; sd = sqrt(sum / P).
 * No fused multiply-add anywhere.
 *
 * state (C, 8) doubles, the record of population c (integers exact): [0] status (1 while running), [1] beta_s, [2] logZ,
 * [3] ESS(beta_s) / P, [4] scale_s, [5] r of the last stage whose step 6 ran, [6] s = the stages done, [7] the accepted steps
 * behind [5].  sx_smc_stage(s) first performs step 6 of stage s - 1 for the populations whose [6] is s - 1, then steps 1 - 3
 * of stage s for those still running; call it once more (s = last + 1 <= maxiter + 1) after the last mutation for that step 6.
 * The host reads the records once per stage to decide whether to go on; nothing else is synchronised.
 * ------------------------------------------------------------------------- */
typedef struct sx_smc_args {
    double *x[2];            /* DEVICE (C P, n) each: the particles of stage s live in x[s & 1]; initialised memory          */
    double *f[2];            /* DEVICE (C P) each: their values                                                             */
    int32_t *anc;            /* DEVICE (C P): the ancestors of the latest stage, indices inside the population              */
    int64_t *nacc;           /* DEVICE (C P): the accepted steps of each particle in the latest mutation                    */
    double *step;            /* DEVICE (C, n): step 4                                                                       */
    double *state;           /* DEVICE (C, 8): the records                                                                  */
    const double *lower, *upper; /* DEVICE (n)                                                                              */
    int64_t C, P;            /* C >= 1, 4 <= P <= sx_smc_max_particles(), C P < 2^31                                        */
    int32_t n, fun_id;       /* 1 <= n <= sx_wide_from(); fun_id is read by sx_smc_init / sx_smc_mutate alone               */
    int32_t steps, maxiter;  /* M >= 1, the most stages >= 1; steps * maxiter < 2^31                                        */
    double ess, target;      /* both in (0, 1)                                                                              */
    double scale;            /* scale_1: finite, > 0                                                                        */
    uint32_t key0, key1;
} sx_smc_args;
/* sizeof(sx_smc_args) as the library was built (sx_struct_size is not extended) */
int sx_smc_args_bytes(void);
/* the most particles of one population: their values fit one workgroup's LDS (160 KiB) */
int sx_smc_max_particles(void);
/* Every entry point below is one launch, checks its arguments as sx_sample_run does (-1 and sx_last_error), and takes the
 * stage s it works on.  stage 0: draw and evaluate the particles into x[0] / f[0], start the records */
int sx_smc_init(const sx_smc_args *a, void *stream);
/* step 6 of stage s - 1, steps 1 - 3 of stage s (1 <= s <= maxiter + 1): state, anc */
int sx_smc_stage(const sx_smc_args *a, int s, void *stream);
/* the rest of step 3 and step 4 (1 <= s <= maxiter): x / f [(s - 1) & 1] through anc -> x / f [s & 1]; step */
int sx_smc_resample(const sx_smc_args *a, int s, void *stream);
/* step 5 with the objective fun_id in the kernel: x / f [s & 1] in place, nacc */
int sx_smc_mutate(const sx_smc_args *a, int s, void *stream);
/* step 5 around a caller-supplied objective, per step m = 1 ... M: propose -> fprop = fun(prop) -> decide; prop (C P, n),
 * fprop (C P) DEVICE.  A frozen particle proposes itself.  Stage 0 is (s, m) = (0, 0): propose draws the particles into prop,
 * decide moves them and fprop into x[0] / f[0] and starts the records.  With bit-identical objective values this is
 * sx_smc_init / sx_smc_mutate's run, bit for bit. */
int sx_smc_propose(const sx_smc_args *a, int s, int m, double *prop, void *stream);
int sx_smc_decide(const sx_smc_args *a, int s, int m, const double *prop, const double *fprop, void *stream);

/* ------------------------------------------------------------------------- *
 * Differential Evolution, many independent runs in one launch (csrc/sx_de_runs.hip).
 * replaces: R calls of de/_de.py:176-301 (`de`: initial population :208-218, the generation loop :236-283) with
 *           de_sync (:314-351), the strategies (de/_strategy.py:1-46), Random (de/_constraints.py:13-28),
 *           selection_sync (_common.py:123-130) and the termination ladder (_common.py:131-158) -- everything a run of
 *           `updating="deferred"` does, for R runs that differ in their Philox key (and, optionally, their x0) only.
 * One workgroup carries one run from its initial population to its termination: both population buffers (generation g
 * in buffer g & 1, as in sx_de_args) and the fitness values live in the workgroup's LDS, a generation is separated from
 * the next by two workgroup barriers, and nothing is exchanged between runs.  Run r draws with keys[r]: its counters
 * are those of the single-run kernels (row = the row within the run), so run r IS the run sx_de_chain_launch performs
 * with that key -- same population, same best, same nit and status, bit for bit.  In-kernel draws only.
 * ------------------------------------------------------------------------- */
typedef struct sx_de_runs_args {
    const uint32_t *keys;   /* DEVICE (R,2) Philox key (key0, key1) of run r                               */
    const double *lower;    /* DEVICE (n)                                                                  */
    const double *upper;    /* DEVICE (n)                                                                  */
    const double *x0;       /* DEVICE initial populations, (P,n) each, run stride x0_stride; NULL: run r draws the
                               Latin hypercube of sx_philox_lhs with keys[r] (_common.py:109-120)          */
    double *xs;             /* DEVICE (R,n) OUT best individual of run r                                   */
    double *funs;           /* DEVICE (R)   OUT its value                                                  */
    int64_t *nits;          /* DEVICE (R)   OUT generations (the reference's `it`; the initial one counts) */
    int32_t *statuses;      /* DEVICE (R)   OUT -1 / 0 / 1 (_common.py:134-158)                            */
    double *xfinal;         /* DEVICE (R,P,n) OUT final population of run r, or NULL                       */
    int64_t R;
    int64_t P;
    int64_t x0_stride;      /* 0 (one population shared by all runs) or P*n                                */
    int32_t n;              /* 1 ... sx_wide_from()                                                        */
    int32_t fun_id;
    int32_t strategy;
    int32_t constraints;    /* 0 none, 1 Random                                                            */
    int32_t maxiter;        /* <= 1: one generation is still run (de/_de.py:236-283)                       */
    int32_t pad;
    double F, CR, xtol, ftol;
} sx_de_runs_args;

/* all R runs, from the initial population to each run's own termination: one launch, R workgroups */
int sx_de_runs_launch(const sx_de_runs_args *a, void *stream);
/* the same launch with settings of run r's own (a sweep): F (mutation, de/_strategy.py:1-38; the reference admits [0, 2],
 * de/_de.py:129-130), CR (recombination, de/_de.py:341-344; [0, 1], :132-133) and strategy (SX_DE_*, de/_strategy.py:41-46)
 * are each DEVICE (R) or NULL; NULL: every run uses the struct's scalar (sx_de_runs_launch is the all-NULL case, the same
 * kernel).  Run r IS the single run with element r of each array and keys[r], bit for bit.  The host cannot read the
 * arrays: the caller keeps them in range.  A strategy element outside SX_DE_RAND1BIN .. SX_DE_BEST2BIN, or one that needs
 * more than P - 1 donors, ends run r at once: funs[r] = NaN, nits[r] = 0, statuses[r] = SX_STATUS_NONE, xs[r] untouched.
 * The struct's own F, CR and strategy are checked as in sx_de_runs_launch, whether or not an array replaces them. */
int sx_de_runs_sweep_launch(const sx_de_runs_args *a, const double *F, const double *CR, const int32_t *strategy,
                            void *stream);
/* bytes of LDS one run of popsize P and row length n needs (host only, no device touched); negative when that is more
 * than a workgroup may declare (160 KiB on gfx950), n > sx_wide_from() or the shape is invalid */
int64_t sx_de_runs_lds_bytes(int64_t P, int n);

/* ------------------------------------------------------------------------- *
 * PSO / CPSO, many independent runs in one launch (csrc/sx_pso_runs.hip).
 * replaces: R calls of cpso/_cpso.py:182-321 (`cpso`: initial swarm :215-247, the generation loop :257-307) with the
 *           mutation (:324-329), pso_sync (:332-361), NoConstraint / Shrink (cpso/_constraints.py:4-10, 44-53),
 *           selection_sync (_common.py:123-130), the termination ladder (_common.py:131-158) and the competitive restart
 *           (:405-426) -- everything a run of `updating="deferred"` does, for R runs that differ in their Philox key (and,
 *           optionally, their x0) only.  pso/_pso.py:9-122 is the same with competitivity None (gamma = 0 here).
 * One workgroup carries one run from its initial swarm to its termination: X, V, pbest, pbestfit and a copy of the best
 * row live in the workgroup's LDS (a swarm too large for that keeps V, which only its owning lanes touch, in `vwork`), a generation is separated from the next by two workgroup barriers (CPSO: up to two
 * more), and nothing is exchanged between runs.  Run r draws with keys[r]: its counters are those of the single-run
 * kernels (row = the row within the run), so run r IS the run sx_pso_generation / sx_pso_graph_create perform with that
 * key -- same swarm, same best, same nit and status, bit for bit.  In-kernel draws only.
 * ------------------------------------------------------------------------- */
typedef struct sx_pso_runs_args {
    const uint32_t *keys;   /* DEVICE (R,2) Philox key (key0, key1) of run r                               */
    const double *lower;    /* DEVICE (n)                                                                  */
    const double *upper;    /* DEVICE (n)                                                                  */
    const double *x0;       /* DEVICE initial swarms, (P,n) each, run stride x0_stride; NULL: run r draws the
                               Latin hypercube of sx_philox_lhs with keys[r] (_common.py:109-120)          */
    double *xs;             /* DEVICE (R,n) OUT best position of run r                                     */
    double *funs;           /* DEVICE (R)   OUT its value                                                  */
    int64_t *nits;          /* DEVICE (R)   OUT generations (the reference's `it`; the initial one counts) */
    int32_t *statuses;      /* DEVICE (R)   OUT -1 / 0 / 1 (_common.py:134-158)                            */
    double *xfinal;         /* DEVICE (R,P,n) OUT final positions of run r, or NULL                        */
    double *pbest_final;    /* DEVICE (R,P,n) OUT final personal bests, or NULL                            */
    double *pbestfit_final; /* DEVICE (R,P)   OUT their values, or NULL                                    */
    double *vwork;          /* DEVICE sx_pso_runs_workspace_bytes(R, P, n) bytes: the velocities of a swarm whose
                               X, V and pbest do not fit the LDS together; may be NULL when that is 0      */
    int64_t R;
    int64_t P;
    int64_t x0_stride;      /* 0 (one swarm shared by all runs) or P*n                                     */
    int32_t n;              /* 1 ... sx_wide_from()                                                        */
    int32_t fun_id;
    int32_t constraints;    /* 0 none, 1 Shrink                                                            */
    int32_t maxiter;        /* <= 1: one generation is still run (cpso/_cpso.py:257-260)                   */
    double w, c1, c2;       /* inertia, cognitivity, sociability                                           */
    double gamma;           /* competitivity; 0: plain PSO, no restart                                     */
    double delta;           /* log(1 + 0.003 P) / max(0.2, log(0.01 maxiter)) (cpso/_cpso.py:215-216)      */
    double xtol, ftol;
} sx_pso_runs_args;

/* all R runs, from the initial swarm to each run's own termination: one launch, R workgroups */
int sx_pso_runs_launch(const sx_pso_runs_args *a, void *stream);
/* the same launch with settings of run r's own (a sweep): w, c1, c2 (inertia, cognitivity, sociability of the velocity
 * update, cpso/_cpso.py:324-329; the reference admits [0, 1], [0, 4], [0, 4], :127-134) and gamma (competitivity of the
 * restart, :405-426; [0, 2], :136-137; 0: run r never restarts) are each DEVICE (R) or NULL; NULL: every run uses the
 * struct's scalar (sx_pso_runs_launch is the all-NULL case, the same kernel).  `delta` stays the struct's: it depends on P
 * and maxiter only (:215-216) and is read by the runs whose gamma is not 0.  Run r IS the single run with element r of
 * each array and keys[r], bit for bit.  The host cannot read the arrays: the caller keeps them in range. */
int sx_pso_runs_sweep_launch(const sx_pso_runs_args *a, const double *w, const double *c1, const double *c2,
                             const double *gamma, void *stream);
/* bytes of LDS one run of popsize P and row length n needs (host only, no device touched); negative when that is more
 * than a workgroup may declare (160 KiB on gfx950), n > sx_wide_from() or the shape is invalid */
int64_t sx_pso_runs_lds_bytes(int64_t P, int n);
/* bytes of device workspace (sx_pso_runs_args.vwork) R such runs need: 0 when X, V and pbest fit the LDS together, else
 * R*P*n*8 for the velocities (host only); negative when sx_pso_runs_lds_bytes(P, n) is */
int64_t sx_pso_runs_workspace_bytes(int64_t R, int64_t P, int n);

/* ------------------------------------------------------------------------- *
 * CMA-ES, many independent runs in one launch (csrc/sx_cma_runs.hip).
 * replaces: R calls of cmaes/_cmaes.py:143-357 (`cmaes`: sampling :232-237, ranking and recombination :272-277, the
 *           evolution paths :280-287, the covariance update :290-295, the step size :298, the decomposition :301-309)
 *           and of `converge` (:360-434, the ten ordered stopping rules incl. the reads of the zero-initialised
 *           history) -- everything a run without constraints does, for R runs that differ in their Philox key and
 *           their initial mean only.
 * One workgroup carries one run from its first generation to its own stopping rule: C, B, D, both paths, the mean and
 * the candidates live in the workgroup's LDS, the steps of a generation are separated by workgroup barriers where the
 * single run (sx_cmaes_generation) has kernel launches, the decomposition is the one-workgroup Jacobi solver of
 * csrc/sx_eigh_small.hpp (the body of sx_eigh for n <= 32) with the same finish (eigenvalues M_jj / |v_j|^2, ascending
 * order, largest component of every eigenvector positive), and nothing is exchanged between runs.  Run r draws with
 * keys[r]: the counters of sx_cmaes_normals (row = the row within the run), so run r samples what the single run of
 * that key samples.  n <= 32 (the one-workgroup solver's range); no Penalize, no history.
 * ------------------------------------------------------------------------- */
typedef struct sx_cma_runs_args {
    const uint32_t *keys;   /* DEVICE (R,2) Philox key (key0, key1) of run r                               */
    const double *xmean0;   /* DEVICE (R,n) initial mean of run r, standardised ((x0 - xm) / xstd)         */
    const double *xm;       /* DEVICE (n) (upper + lower) / 2                         (cmaes/_cmaes.py:167-173) */
    const double *xstd;     /* DEVICE (n) (upper - lower) / 2                                              */
    const double *w;        /* DEVICE (mu) recombination weights                              (:184-196)   */
    double *work;           /* DEVICE sx_cma_runs_workspace_bytes(R, maxiter) bytes: the runs' best-fitness histories;
                               zeroed by sx_cma_runs_launch                                                */
    double *xs;             /* DEVICE (R,n) OUT best candidate of run r's last generation, un-standardised */
    double *funs;           /* DEVICE (R)   OUT its value                                                  */
    int64_t *nits;          /* DEVICE (R)   OUT generations                                                */
    int32_t *statuses;      /* DEVICE (R)   OUT the reference's status (-8 .. 1)                           */
    int64_t *nfevs;         /* DEVICE (R)   OUT nit * P, or NULL                                           */
    double *sigmas;         /* DEVICE (R)   OUT final step size, or NULL                                   */
    double *xmeans;         /* DEVICE (R,n) OUT final mean (standardised), or NULL                         */
    int64_t R;
    int64_t P;
    int32_t n;              /* 1 ... 32                                                                    */
    int32_t mu;
    int32_t fun_id;
    int32_t maxiter;        /* >= 1                                                                        */
    int32_t ilim;           /* int(10 + 30 n / P): window of stopping rule -5                    (:399)    */
    int32_t pad;
    double mueff, cc, cs, c1, cmu, damps, chind;  /* strategy constants                       (:184-205)   */
    double sigma;           /* initial step size                                                           */
    double insigma;         /* the step size rules -6 and -8 compare with (the single run: the same value) */
    double xtol, ftol;
} sx_cma_runs_args;

/* all R runs, from the first generation to each run's own stopping rule: one launch, R workgroups */
int sx_cma_runs_launch(const sx_cma_runs_args *a, void *stream);
/* the same launch with an initial step size of run r's own (a sweep): sigma (cmaes/_cmaes.py:222; > 0, :109-110) is
 * DEVICE (R) or NULL; NULL: every run uses the struct's sigma and insigma (sx_cma_runs_launch is that case, the same
 * kernel).  With an array, sigma[r] is both the step size run r starts from and the `insigma` its stopping rules -6 and
 * -8 compare with (:418, :431), as in the single run.  The host cannot read the array: the caller keeps it positive. */
int sx_cma_runs_sweep_launch(const sx_cma_runs_args *a, const double *sigma, void *stream);
/* bytes of LDS one run of popsize P and dimension n needs (host only, no device touched; the layout is written out at
 * the head of csrc/sx_cma_runs.hip); negative when that is more than a workgroup may declare (160 KiB on gfx950),
 * n < 1, n > 32 or P < 2 */
int64_t sx_cma_runs_lds_bytes(int64_t P, int n);
/* bytes of device workspace (sx_cma_runs_args.work) R runs of at most maxiter generations need: R*maxiter*8 (host
 * only); negative for R < 1 or maxiter < 1 */
int64_t sx_cma_runs_workspace_bytes(int64_t R, int64_t maxiter);

/* ------------------------------------------------------------------------- *
 * VD-CMA, many independent runs in one launch (csrc/sx_vd_runs.hip).
 * replaces: R calls of vdcma/_vdcma.py:144-425 (`vdcma`: candidates and mean-shift injection :236-248, ranking and mean
 *           shift :289-295, rank-gap step size :298-306, evolution path and model constants :309-328, moments :331-345
 *           and :428-444, natural gradient and the update of v and d :348-378 and :447-460) and of `converge`
 *           (cmaes/_cmaes.py:360-434 without B and D) -- everything a run without constraints does, for R runs that
 *           differ in their Philox key, their initial mean and their initial direction only.
 * One workgroup carries one run from its first generation to its own stopping rule: d, v, pc, the mean and the steps'
 * by-products live in the workgroup's LDS; neither the candidates nor the steps are stored -- a step is formed again from
 * its normals (a function of the counter) where it is needed --, so the LDS is O(n + P) and runs of hundreds of variables
 * fit.  Run r draws with keys[r]: the counters of sx_cmaes_normals (row = the row within the run, the injection's normals
 * "row P"), so run r samples what the single run of that key samples.  6 <= n; no Penalize, no history.
 * ------------------------------------------------------------------------- */
typedef struct sx_vd_runs_args {
    const uint32_t *keys;   /* DEVICE (R,2) Philox key (key0, key1) of run r                               */
    const double *xmean0;   /* DEVICE (R,n) initial mean of run r, standardised ((x0 - xm) / xstd)         */
    const double *vvec0;    /* DEVICE (R,n) initial direction v of run r                       (:207)      */
    const double *xm;       /* DEVICE (n) (upper + lower) / 2                         (cmaes/_cmaes.py:167-173) */
    const double *xstd;     /* DEVICE (n) (upper - lower) / 2                                              */
    const double *w;        /* DEVICE (mu) recombination weights                              (:185-191)   */
    double *work;           /* DEVICE sx_vd_runs_workspace_bytes(R, maxiter) bytes: the runs' best-fitness histories;
                               zeroed by sx_vd_runs_launch                                                 */
    double *xs;             /* DEVICE (R,n) OUT best candidate of run r's last generation, un-standardised */
    double *funs;           /* DEVICE (R)   OUT its value                                                  */
    int64_t *nits;          /* DEVICE (R)   OUT generations                                                */
    int32_t *statuses;      /* DEVICE (R)   OUT the reference's status (-8 .. 1)                           */
    int64_t *nfevs;         /* DEVICE (R)   OUT nit * P, or NULL                                           */
    double *sigmas;         /* DEVICE (R)   OUT final step size, or NULL                                   */
    double *xmeans;         /* DEVICE (R,n) OUT final mean (standardised), or NULL                         */
    double *dvecs;          /* DEVICE (R,n) OUT final d, or NULL                                           */
    double *vvecs;          /* DEVICE (R,n) OUT final v, or NULL                                           */
    int64_t R;
    int64_t P;
    int32_t n;              /* 6 ... what sx_vd_runs_lds_bytes admits                                      */
    int32_t mu;
    int32_t fun_id;
    int32_t maxiter;        /* >= 1                                                                        */
    int32_t ilim;           /* int(10 + 30 n / P): window of stopping rule -5                              */
    int32_t pad;
    double mueff, cc, c1, cmu, cs, ds, wsum;  /* strategy constants (:185-199); cs = 0.3, ds = sqrt(n), wsum = sum(w) */
    double sigma;           /* initial step size                                                           */
    double insigma;         /* the step size rules -6 and -8 compare with (the single run: the same value) */
    double xtol, ftol;
} sx_vd_runs_args;

/* all R runs, from the first generation to each run's own stopping rule: one launch, R workgroups */
int sx_vd_runs_launch(const sx_vd_runs_args *a, void *stream);
/* the same launch with an initial step size of run r's own (a sweep): sigma (vdcma/_vdcma.py:229; > 0, :110-111) is
 * DEVICE (R) or NULL; NULL: every run uses the struct's sigma and insigma (sx_vd_runs_launch is that case, the same
 * kernel).  With an array, sigma[r] is both the step size run r starts from and the `insigma` its stopping rules -6 and
 * -8 compare with (cmaes/_cmaes.py:418, :431), as in the single run.  The host cannot read the array: the caller keeps it
 * positive. */
int sx_vd_runs_sweep_launch(const sx_vd_runs_args *a, const double *sigma, void *stream);
/* sizeof(sx_vd_runs_args) as the library was built (sx_struct_size is not extended) */
int sx_vd_runs_args_bytes(void);
/* bytes of LDS one run of popsize P and dimension n needs (host only, no device touched; the layout is written out at
 * the head of csrc/sx_vd_runs.hip); negative when that is more than a workgroup may declare (160 KiB on gfx950),
 * n < 6, n > sx_wide_from() or P < 2 */
int64_t sx_vd_runs_lds_bytes(int64_t P, int n);
/* bytes of device workspace (sx_vd_runs_args.work) R runs of at most maxiter generations need: R*maxiter*8 (host
 * only); negative for R < 1 or maxiter < 1 */
int64_t sx_vd_runs_workspace_bytes(int64_t R, int64_t maxiter);

/* ------------------------------------------------------------------------- *
 * DE and PSO, many independent runs around a CALLER-SUPPLIED ROW-WISE objective (csrc/sx_runs_unfused.hip): the batched
 * counterpart of sx_de_propose / sx_pso_move / sx_rows_select / sx_select_finalize above.  The objective cannot be fused,
 * so the R populations live in device memory -- three (R,P,n) arrays -- and a generation of ALL runs is
 *   sx_runs_rowwise_de_propose / _pso_move -> the caller's objective, once, on the stacked (R*P, n) rows ->
 *   sx_runs_rowwise_select -> sx_runs_rowwise_finalize.
 * Row r*P + i is individual i of run r.  Stacking is only correct for an objective whose value of a row depends on that row
 * alone (factory.batched(f, rowwise=True)).
 * Geometry: the row geometry of the single-run kernels (sx_rows_per_workgroup(n) rows a workgroup), and a workgroup never
 * spans two runs: a run takes sx_runs_rowwise_partials(P, n) = ceil(P / sx_rows_per_workgroup(n)) workgroups, workgroup b
 * serves run b / that number, so a run's (part_f, part_i) records are those of the single run.  Run r draws with keys[r]; the
 * Philox counters are those of the single-run kernels (row = the row within the run, generation = state[r].it + 1), the
 * arithmetic and the orders of summation too: given the same objective values, run r IS the single run of its key -- same
 * population, best, nit and status, bit for bit.  In-kernel draws only.  A run that has ended (state[r].done) is frozen: every
 * kernel returns at entry for its workgroups, so its rows of the stacked tensor keep their last contents.
 * ------------------------------------------------------------------------- */
typedef struct sx_runs_rowwise_args {
    const uint32_t *keys;   /* DEVICE (R,2) Philox key (key0, key1) of run r                               */
    const double *lower;    /* DEVICE (n)                                                                  */
    const double *upper;    /* DEVICE (n)                                                                  */
    const double *x0;       /* DEVICE initial populations, (P,n) each, run stride x0_stride; NULL: run r draws the
                               Latin hypercube of sx_philox_lhs with keys[r] (_common.py:109-120)          */
    double *pop0;           /* DEVICE (R,P,n)  DE: population buffer 0 (generation g of run r lives in buffer g & 1, g =
                               state[r].it, as in sx_de_args)           PSO: X, the rows the objective is handed   */
    double *pop1;           /* DEVICE (R,P,n)  DE: population buffer 1                       PSO: V                */
    double *pop2;           /* DEVICE (R,P,n)  DE: cand, the rows the objective is handed    PSO: pbest            */
    double *fit;            /* DEVICE (R*P)    DE: fitness of the current rows               PSO: pbestfit         */
    double *candfit;        /* DEVICE (R*P)    the values of the last evaluated rows (as sx_de_args.candfit)      */
    const double *f;        /* DEVICE (R*P)    IN what the objective returned for the rows it was handed: read by _start
                               and _select only, and may point elsewhere in every call (NULL for the others)       */
    sx_state *state;        /* DEVICE (R)      run r's generation state (64 bytes each)                            */
    double *gbest;          /* DEVICE (R,n)    run r's best row                                                    */
    double *part_f;         /* DEVICE (R, sx_runs_rowwise_partials(P,n)) per-workgroup records of the selection    */
    int64_t *part_i;        /* DEVICE (same)   their rows, within the run                                          */
    double *xs;             /* DEVICE (R,n) OUT best individual of run r, written when the run ends                */
    double *funs;           /* DEVICE (R)   OUT its value                                                          */
    int64_t *nits;          /* DEVICE (R)   OUT generations (the reference's `it`; the initial one counts)         */
    int32_t *statuses;      /* DEVICE (R)   OUT -1 / 0 / 1 (_common.py:134-158)                                    */
    int32_t *ended;         /* DEVICE (1)   IN/OUT number of runs that have ended (zeroed by the caller; a run adds
                               one when it ends): what the host reads to learn whether any run is still active     */
    int64_t R;
    int64_t P;              /* >= 2; R*P < 2^31                                                                    */
    int64_t x0_stride;      /* 0 (one population shared by all runs) or P*n                                        */
    int32_t n;              /* 1 ... sx_wide_from()                                                                */
    int32_t method;         /* 0 DE, 1 PSO                                                                         */
    int32_t strategy;       /* DE                                                                                  */
    int32_t constraints;    /* 0 none, 1 Random (DE) / Shrink (PSO)                                                */
    int32_t maxiter;        /* <= 1: one generation is still run                                                   */
    int32_t pad;
    double F, CR;           /* DE                                                                                  */
    double w, c1, c2;       /* PSO                                                                                 */
    double xtol, ftol;
} sx_runs_rowwise_args;

/* records (= workgroups) per run: ceil(P / sx_rows_per_workgroup(n)), as sx_num_partials for one run (host only, no device
 * touched); negative for P < 2, n < 1 or n > sx_wide_from() */
int64_t sx_runs_rowwise_partials(int64_t P, int n);
/* the initial populations: with x0 == NULL every run's Latin hypercube under its own key (_common.py:109-120), else x0.
 * replaces: de/_de.py:208-211 (DE: into buffer 1 and into cand, so the objective never sees memory nobody wrote) and
 *           cpso/_cpso.py:219-232 (PSO: X, V = 0, pbest = X).  Touches neither state nor f. */
int sx_runs_rowwise_init(const sx_runs_rowwise_args *a, void *stream);
/* after the objective has evaluated the initial rows (a->f).  replaces: de/_de.py:212-218, cpso/_cpso.py:233-247: fit (DE) /
 * pbestfit (PSO) and candfit <- f; per run the first-minimum argmin of its P values (np.argmin's rules for NaN, +-inf
 * and ties, as sx_argmin); state[r] = {it 1, gbidx, gfit, dx 0, SX_STATUS_NONE, done 0}; gbest[r] <- the best row.
 * strategy: DEVICE (R) or NULL, as in sx_runs_rowwise_de_propose; an element outside SX_DE_RAND1BIN .. SX_DE_BEST2BIN, or one
 * that needs more than P - 1 donors, ends run r here as sx_de_runs_sweep_launch documents (funs[r] = NaN, nits[r] = 0,
 * statuses[r] = SX_STATUS_NONE, xs[r] untouched; counted in *ended). */
int sx_runs_rowwise_start(const sx_runs_rowwise_args *a, const int32_t *strategy, void *stream);
/* DE: pop2 (cand) <- the trial vectors of every running run's generation state[r].it + 1.
 * replaces: de/_de.py:314-351 de_sync up to the candidates (:333-344), de/_strategy.py:1-46, de/_constraints.py:13-28 --
 * sx_de_propose's in-kernel-draw branch per run: donors from the run's own P rows, the best row from gbest[r].  F, CR,
 * strategy: DEVICE (R) or NULL (every run uses the struct's scalar), as in sx_de_runs_sweep_launch. */
int sx_runs_rowwise_de_propose(const sx_runs_rowwise_args *a, const double *F, const double *CR, const int32_t *strategy,
                               void *stream);
/* PSO: pop1 (V) and pop0 (X) of every running run updated in place.
 * replaces: cpso/_cpso.py:324-329 (mutation, left to right), cpso/_constraints.py:4-10, 44-53 (NoConstraint / Shrink, sync
 * form) -- sx_pso_move's in-kernel-draw branch per run; with Shrink the raw velocities wait in the workgroup's LDS for the
 * row-wide beta.  w, c1, c2: DEVICE (R) or NULL, as in sx_pso_runs_sweep_launch. */
int sx_runs_rowwise_pso_move(const sx_runs_rowwise_args *a, const double *w, const double *c1, const double *c2,
                             void *stream);
/* selection after the evaluation (a->f), per running run.  replaces: _common.py:123-130 selection_sync, strict <:
 * DE writes the winner or the old row into the other population buffer; PSO updates pbest in place; candfit <- f; one
 * (part_f, part_i) record per workgroup -- sx_rows_select per run. */
int sx_runs_rowwise_select(const sx_runs_rowwise_args *a, void *stream);
/* best and termination of that generation, one workgroup of 256 threads per run.  replaces: _common.py:131-158 (argmin, the
 * step of the best, the status ladder) -- sx_select_finalize per run, its dx summed in the same order: gbest[r] and state[r]
 * updated; a run that ends writes xs[r], funs[r], nits[r], statuses[r] and adds one to *ended. */
int sx_runs_rowwise_finalize(const sx_runs_rowwise_args *a, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* STOCHOPY_HIP_H */
