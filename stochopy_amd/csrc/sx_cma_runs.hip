// Many independent CMA-ES runs in one launch: one workgroup per run, resident from the first generation to the run's own
// stopping rule (include/stochopy_hip.h, sx_cma_runs_args).  A run of the reference's default size (popsize 4 + 3 ln n) is a
// dozen launches per generation, each a fraction of one workgroup, with a one-workgroup eigensolver between them; R such
// runs under R seeds fill the device instead, and a generation costs ten workgroup barriers plus the decomposition's.
//
// Reference code replaced (paths relative to the reference checkout), R times over:
//   stochopy/optimize/cmaes/_cmaes.py:226-343   the generation loop: sampling (:232-237), objective (:258), ranking and
//                                               recombination (:272-277), paths (:280-287), covariance (:290-295), step
//                                               size (:298), decomposition when due (:301-309)
//   stochopy/optimize/cmaes/_cmaes.py:360-434   converge: the ten ordered stopping rules, incl. the reads of the
//                                               zero-initialised history
//
// LDS of a run (doubles; ldn = n | 1, S = gen_row_stride(n) = n + 8, M2 = 16 for n <= 16 else 32), in this order:
//   C[n][ldn] | B[n][ldn] | D[n] xmean[n] xold[n] ps[n] pc[n] xbest[n] step[n] y[n] isc[n] | lam[M2] scl[M2] inv[M2] |
//   fit[P] | order[P] as int32, (P + 1) / 2 doubles | red[24]: block_sum's 17 partials | part[8][4]: the waves' history
//   and fitness extremes | U = max(P * S, 4 * M2 * (M2 + 1) + 2 * M2)
// = 2 n ldn + 9 n + 3 M2 + P + (P + 1) / 2 + 56 + max(P S, 4 M2 (M2 + 1) + 2 M2) doubles (sx_cma_runs_lds_bytes).
// U holds the candidates arx[P][S] -- a row is the staging area row_objective wants, so a candidate is built, evaluated
// (un-standardised in place, then put back) and kept where it is -- and, during a decomposition, the Jacobi solver's
// storage (S[2], W[2]: [M2][M2 + 1] each, c[M2], s[M2]).  The lifetimes do not overlap: the candidates are dead once the
// covariance update has read the mu best of them (the best row, which the result needs, is copied to xbest before), and
// the decomposition follows that update; the next generation's sampling rewrites every row.
// The best-fitness history (besthist[maxiter], read by stopping rules -5 and -7) is the run's slice of the caller's
// workspace, zeroed by sx_cma_runs_launch: entry `gen` is read before it is written, as in the reference (cma_stop_kernel).
//
// A generation mirrors sx_cmaes_generation (sx_cma_loop.hip) with barriers where it has launches: the same normals (the
// device function behind sx_cmaes_normals, counter (slot, row, gen, kPurposeCmaNormal), row = the row within the run), the
// same objective (row_objective<FUN, 16> on the un-standardised row), key_less for the ranking, the expressions of
// cma_paths_kernel / cma_cov_finish_kernel, the stopping rules as sx_cma_rules.hpp states them for cma_stop_kernel (spelled
// out here: see LEFT APART below), the sweeps of eigh_small_kernel (sx_eigh_small.hpp: rotation,
// jacobi_sweep, block_sum; cold start, tol = max(1e-14, n 2^-53), kRunsSweeps sweeps at the most) and the finish of
// eigh_colstats / eigh_rank / eigh_write_kernel.  Sums whose order the single run leaves to its launch geometry (dot
// products with B, the recombination, the covariance contraction) are summed here in index order, which depends on n and mu
// only: run r agrees with the single run of its key to rounding, not bit for bit, and with the oracle as the single run does.
// The loop that drives the sweeps (measure, compare, sweep) is the one statement sequence that exists twice
// (eigh_small_kernel keeps its own: as a shared function it compiled to other instructions there).
// LEFT APART from sx_cma_rules.hpp, on measurement (profiles/cma_rules_refactor_resources.txt and
// cma_rules_refactor_ab.txt): this kernel keeps its own spelling of history_extremes, rule_facts_add and cma_stop_status,
// and the ranking by wave votes stands here and in vd_runs_kernel (sx_vd_runs.hip); it compiles to the instructions it had
// before that header existed.  It sits at 128 VGPRs with 568 ... 812 bytes of scratch per lane: history_extremes,
// cma_stop_status or the votes as a shared function -- each alone, together, as values, by reference, with early returns --
// made 1 ... 5 of the 14 instantiations GAIN 4 ... 36 bytes of scratch; rule_facts_add alone cost no register, gave the
// same bytes, and ran 0.11 ... 0.16 % below the parent's own spread at n = 32 with 4096 and 16 384 runs, twice.
// A correction to a rule in the header is owed here as well.
// What return_all would need (the argmin row of cma_rank_kernel) has no reader here and is not computed: the result is the
// first row of the ranking, as in cma_stop_kernel.
//
// Nothing passes between workgroups: no grid barrier, no spin-wait, no atomics.  Every loop is bounded by maxiter,
// kRunsSweeps, P, mu or n.
#include "sx_device.hpp"
#include "sx_eigh_small.hpp"
#include "sx_host.hpp"
#include "sx_rowops.hpp"
#include "sx_runs.hpp"

using namespace sx;

namespace {

constexpr int kRunsMaxDim = 32;            // the one-workgroup solver's range (sx_eigh.hip kSmallPathMax)
constexpr int kRunsSweeps = 40;            // what the single run allows a decomposition started from the identity (COLD_SWEEPS)
constexpr int kRunsLpr = 16;               // lanes per candidate row (lanes_per_row(n) for n <= 64)
constexpr int kRedWords = 24, kPartWaves = 8, kPartWords = 4;
static_assert(kRunsSweeps <= kEighMaxSweeps, "the solver's own cap");

template <int M2>
constexpr int runs_threads() {  // enough rows in flight for the sampling, and every thread the Jacobi sweep needs
    return M2 == 16 ? 256 : 512;
}
static_assert(runs_threads<16>() >= jacobi_threads<16>() && runs_threads<32>() >= jacobi_threads<32>(), "Jacobi threads");
static_assert(runs_threads<32>() / kWave <= kPartWaves, "part[] rows");

__host__ __device__ inline int runs_m2(int n) { return n <= 16 ? 16 : 32; }

struct RunsLayout {  // offsets in doubles (see the header comment)
    int C, B, vec, ev, fit, order, red, part, U, total;
};
__host__ __device__ inline RunsLayout runs_layout(int64_t P, int n) {
    const int ldn = n | 1, m2 = runs_m2(n);
    const int64_t cand = P * (int64_t)gen_row_stride(n), jac = 4 * m2 * (m2 + 1) + 2 * m2;
    RunsLayout L;
    L.C = 0;
    L.B = L.C + n * ldn;
    L.vec = L.B + n * ldn;
    L.ev = L.vec + 9 * n;
    L.fit = L.ev + 3 * m2;
    L.order = L.fit + (int)P;
    L.red = L.order + (int)((P + 1) / 2);
    L.part = L.red + kRedWords;
    L.U = L.part + kPartWaves * kPartWords;
    L.total = L.U + (int)(cand > jac ? cand : jac);
    return L;
}

// minimum wavefronts per SIMD asked of the compiler: 4 caps the kernels at 128 VGPRs (two workgroups of 512 threads, four
// of 256 per CU), as in de_runs_kernel / pso_runs_kernel
#ifndef SX_CMA_RUNS_WAVES
#define SX_CMA_RUNS_WAVES 4
#endif
template <int FUN, int M2>
__global__ __launch_bounds__(runs_threads<M2>(), SX_CMA_RUNS_WAVES) void cma_runs_kernel(const sx_cma_runs_args a, const PlanArg plan,
                                                                                         const SigmaSweep sw) {
    constexpr int NT = runs_threads<M2>(), NW = NT / kWave, LPR = kRunsLpr, RPP = NW * (kWave / LPR), LDJ = M2 + 1;
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int64_t run = blockIdx.x;
    const int n = a.n, P = (int)a.P, mu = a.mu, maxiter = a.maxiter;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, l = lane & (LPR - 1), slot = wave * (kWave / LPR) + lane / LPR;
    const int ldn = n | 1, S = gen_row_stride(n);
    const RunsLayout Lo = runs_layout(P, n);
    double *const C = lds + Lo.C, *const B = lds + Lo.B;
    double *const D = lds + Lo.vec, *const xmean = D + n, *const xold = xmean + n, *const ps = xold + n, *const pc = ps + n;
    double *const xbest = pc + n, *const step = xbest + n, *const yv = step + n, *const isc = yv + n;
    double *const lam = lds + Lo.ev, *const scl = lam + M2;
    int *const inv = reinterpret_cast<int *>(scl + M2);
    double *const fit = lds + Lo.fit;
    int *const order = reinterpret_cast<int *>(lds + Lo.order);
    double *const red = lds + Lo.red, *const part = lds + Lo.part;
    double *const arx = lds + Lo.U;
    // the solver's storage, over the (then dead) candidates
    double *const jS = lds + Lo.U, *const jW = jS + 2 * M2 * LDJ, *const jc = jW + 2 * M2 * LDJ, *const js = jc + M2;
    const JacobiView J{jS, jS + M2 * LDJ, jW, jW + M2 * LDJ, jc, js};
    double *const hist = a.work + run * (int64_t)maxiter;  // zeroed by the launch function
    const uint32_t key0 = a.keys[2 * run], key1 = a.keys[2 * run + 1];

    // ---- the model a run starts from (cmaes/_cmaes.py:207-224): C = B = I, D = 1, paths 0, the caller's mean
    for (int t = tid; t < n * ldn; t += NT) {
        const double v = (t / ldn == t % ldn) ? 1.0 : 0.0;
        C[t] = v, B[t] = v;
    }
    for (int e = tid; e < n; e += NT) {
        D[e] = 1.0, xmean[e] = a.xmean0[run * n + e], xold[e] = 0.0, ps[e] = 0.0, pc[e] = 0.0;
    }
    // what a lane of a candidate row needs of the standardisation: its elements l and l + 16
    const int e0 = l, e1 = l + LPR;
    const double xs0 = e0 < n ? a.xstd[e0] : 0.0, xm0 = e0 < n ? a.xm[e0] : 0.0;
    const double xs1 = e1 < n ? a.xstd[e1] : 0.0, xm1 = e1 < n ? a.xm[e1] : 0.0;
    const double cs = a.cs, cc = a.cc, c1 = a.c1, cmu = a.cmu, mueff = a.mueff;
    const double kps = sqrt(cs * (2.0 - cs) * mueff), kpc = sqrt(cc * (2.0 - cc) * mueff);
    const double decay = 1.0 - c1 - cmu;
    const double tol = fmax(1.0e-14, (double)n * 1.1102230246251565e-16);  // as cma_model_update passes it
    // the run's own initial step size: a sweep's element `run`, else the struct's.  Rules -6 and -8 compare with it
    // (`insigma`).  WHERE that value is read decides nothing but the register allocation of a kernel that sits at its SGPR and
    // VGPR limits, and that is measurable: read at entry and kept over the generation loop for the narrow solver, read again
    // where the rules use it for the wide one (either way alone costs one of the widths 2 ... 7 %)
    constexpr bool kInsigmaAtEntry = M2 == 16;
    const double insigma_entry = kInsigmaAtEntry ? run_setting(sw.sigma, run, a.insigma) : 0.0;
    double sigma = run_setting(sw.sigma, run, a.sigma);  // (uniform: every thread works it out from the same LDS values)
    int64_t eigeneval = 0;
    __syncthreads();

    for (int gen = 1; gen <= maxiter; ++gen) {  // (generation maxiter ends with status -1 at the latest)
        // ---- candidates (:232-237) and their objective (:258): arx = xmean + sigma * B (D o z), row by row
        for (int row = slot; row < P; row += RPP) {
            double *U = arx + (size_t)row * S;
            double z0 = 0.0, z1 = 0.0;
            // elements l and l + 16 are the cosine and the sine half of ONE call (slot l): cma_normals_kernel's layout for
            // rows of up to 32 elements
            if (e0 < n) cma_normal_pair((uint32_t)l, (uint32_t)row, (uint32_t)gen, key0, key1, z0, z1);
            if (e0 < n) U[e0] = D[e0] * z0;
            if (e1 < n) U[e1] = D[e1] * z1;
            lds_wave_fence();
            double v0 = 0.0, v1 = 0.0;
            if (e0 < n) {
                double acc = 0.0;
                for (int j = 0; j < n; ++j) acc += B[e0 * ldn + j] * U[j];
                v0 = xmean[e0] + sigma * acc;
            }
            if (e1 < n) {
                double acc = 0.0;
                for (int j = 0; j < n; ++j) acc += B[e1 * ldn + j] * U[j];
                v1 = xmean[e1] + sigma * acc;
            }
            lds_wave_fence();  // every lane of the row has read D o z
            if (e0 < n) U[e0] = v0 * xs0 + xm0;  // cmaes/_cmaes.py:171 unstandardize
            if (e1 < n) U[e1] = v1 * xs1 + xm1;
            const double f = row_objective<FUN, LPR>(U, n, plan, l);
            lds_wave_fence();  // every lane of the row has read the staged point
            if (e0 < n) U[e0] = v0;
            if (e1 < n) U[e1] = v1;
            if (l == 0) fit[row] = f;
        }
        __syncthreads();

        // ---- order = argsort(fit) (:272; NaN last, lower index first on ties): cma_rank_kernel's votes, a wavefront
        //      ranks four rows against 64-key chunks (the same loop as in vd_runs_kernel: see the header comment)
        for (int g = wave; 4 * g < P; g += NW) {
            const int i0 = 4 * g;
            double fi[4];
            int cnt[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) fi[u] = i0 + u < P ? fit[i0 + u] : 0.0, cnt[u] = 0;
            for (int k0 = 0; k0 < P; k0 += kWave) {  // uniform trip count: every lane adds every vote
                const int k = k0 + lane;
                const bool in = k < P;
                const double fk = in ? fit[k] : 0.0;
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const bool front = in && (key_less(fk, fi[u]) || (!key_less(fi[u], fk) && k < i0 + u));
                    cnt[u] += (int)__popcll(__ballot(front));
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (lane == u && i0 + u < P) order[cnt[u]] = i0 + u;
        }
        __syncthreads();
        const int best_row = order[0];
        const double fbest = fit[best_row];
        if (tid == 0) hist[gen - 1] = fbest;

        // ---- xold = xmean; xmean = w @ arx[order[:mu]] (:273-274); the best row aside (the result reads it after the
        //      candidates are gone)
        for (int e = tid; e < n; e += NT) {
            const double xo = xmean[e];
            double xn = 0.0;
            for (int k = 0; k < mu; ++k) xn += a.w[k] * arx[(size_t)order[k] * S + e];
            xold[e] = xo, xmean[e] = xn, step[e] = xn - xo;
            xbest[e] = arx[(size_t)best_row * S + e];
        }
        __syncthreads();
        // ---- C^(-1/2) step as B ((B^T step) / D), then ps (:280-282)
        for (int j = tid; j < n; j += NT) {
            double acc = 0.0;
            for (int i = 0; i < n; ++i) acc += B[i * ldn + j] * step[i];
            yv[j] = acc / D[j];
        }
        __syncthreads();
        for (int i = tid; i < n; i += NT) {
            double acc = 0.0;
            for (int j = 0; j < n; ++j) acc += B[i * ldn + j] * yv[j];
            isc[i] = acc;
            ps[i] = (1.0 - cs) * ps[i] + kps * acc / sigma;
        }
        __syncthreads();
        // ---- |ps|, cond, pc, the step size to come, the coefficient of :291 -- cma_paths_kernel's expressions
        double q2 = 0.0;
        for (int e = 0; e < n; ++e) q2 += ps[e] * ps[e];
        const double psn = sqrt(q2);
        // cond = |ps| / sqrt(1 - (1-cs)^(2 nfev / P)) / chind < 1.4 + 2/(n+1)   with nfev = gen * P      :283-285
        const bool cond = psn / sqrt(1.0 - pow(1.0 - cs, 2.0 * (double)gen)) / a.chind < 1.4 + 2.0 / (n + 1.0);
        for (int e = tid; e < n; e += NT) {
            double p = pc[e] * (1.0 - cc);            // :286
            if (cond) p += kpc * step[e] / sigma;     // :287
            pc[e] = p;
        }
        const double tmp_coef = cond ? 0.0 : c1 * cc * (2.0 - cc);                      // :291
        const double sigma_next = sigma * exp((cs / a.damps) * (psn / a.chind - 1.0));  // :298
        // artmp = (arx[order[:mu]] - xold) / sigma (:290), in place: those rows have no other reader left
        for (int t = tid; t < mu * n; t += NT) {
            const int k = t / n, e = t % n;
            double *p = arx + (size_t)order[k] * S + e;
            *p = (*p - xold[e]) / sigma;
        }
        __syncthreads();
        // ---- covariance (:290-295), upper triangle, mirrored: the operations of cma_cov_finish_kernel in their order
        for (int t = tid; t < n * n; t += NT) {
            const int i = t / n, j = t % n;
            if (i > j) continue;
            double g = 0.0;
            for (int k = 0; k < mu; ++k) {
                const double *yr = arx + (size_t)order[k] * S;
                g += (yr[i] * a.w[k]) * yr[j];
            }
            const double cold = C[i * ldn + j];
            double c = cold * decay;
            c = c + cmu * g;
            c = c + c1 * (pc[i] * pc[j]);
            c = c + tmp_coef * cold;
            C[i * ldn + j] = c;
            if (i != j) C[j * ldn + i] = c;
        }
        __syncthreads();

        // ---- decomposition when due (:301-309; decomposition_due of optimize/_cmaes.py, the run's own eigeneval)
        if ((double)((int64_t)gen * P - eigeneval) > (double)P / (c1 + cmu) / (double)n / 10.0) {  // (uniform)
            eigeneval = (int64_t)gen * P;
            double n2 = 0.0;
            for (int e = tid; e < M2 * M2; e += NT) {
                const int i = e / M2, j = e % M2;
                double v = 0.0;
                if (i < n && j < n) v = i <= j ? C[i * ldn + j] : C[j * ldn + i];
                jS[i * LDJ + j] = v;
                jW[i * LDJ + j] = i == j ? 1.0 : 0.0;
                n2 += v * v;
            }
            int cur, sw, conv;
            double thr2;
            eigh_small_sweeps<M2, NT>(J, jS, red, kRunsSweeps, tol, tid, cur, sw, conv, n2, thr2, [](int, double) {});
            const double *Mf = jS + cur * (M2 * LDJ), *Vf = jW + cur * (M2 * LDJ);
            // per column j of V: |v_j|^2, the sign of its largest-magnitude component (lowest row on ties);
            // lam = M_jj / |v_j|^2, scl = sign / |v_j| (eigh_colstats_kernel)
            for (int j = tid; j < n; j += NT) {
                double tot = 0.0, mx = -1.0, sg = 1.0;
                for (int i = 0; i < n; ++i) {
                    const double v = Vf[i * LDJ + j];
                    tot += v * v;
                    const double av = fabs(v);
                    if (av > mx) mx = av, sg = v < 0.0 ? -1.0 : 1.0;
                }
                lam[j] = Mf[j * LDJ + j] / tot;
                scl[j] = sg / sqrt(tot);
            }
            __syncthreads();
            // ascending rank (ties: lower position first; eigh_rank_kernel); D = sqrt(eigenvalues) (:306)
            for (int j = tid; j < n; j += NT) {
                const double lj = lam[j];
                int rank = 0;
                for (int k = 0; k < n; ++k) {
                    const double lk = lam[k];
                    rank += (lk < lj || (lk == lj && k < j)) ? 1 : 0;
                }
                inv[rank] = j;
                D[rank] = sqrt(lj);
            }
            __syncthreads();
            // B[i][r] = V[i][inv[r]] * scl[inv[r]] (eigh_write_kernel)
            for (int t = tid; t < n * n; t += NT) {
                const int i = t / n, r = t % n, j = inv[r];
                B[i * ldn + r] = Vf[i * LDJ + j] * scl[j];
            }
            __syncthreads();
        }

        // ---- the ten ordered stopping rules (:360-434): history_extremes and, below, rule_facts_add and cma_stop_status of
        //      sx_cma_rules.hpp, spelled out (see the header comment).  "all(x < t)" is carried as the count of elements that
        //      FAIL (NaN fails, as in numpy); entry `gen` of the zero-initialised history is read before it is written.
        //      Every wavefront folds its share of the histories, the totals are folded by everybody
        sigma = sigma_next;
        {
            double wmax = -__builtin_inf(), wmin = __builtin_inf(), jmax = -__builtin_inf(), jmin = __builtin_inf();
            if (gen >= a.ilim) {
                const int hi = gen + 1 < maxiter ? gen + 1 : maxiter;
                for (int k = gen - a.ilim + tid; k < hi; k += NT) {
                    const double v = hist[k];
                    wmax = fmax(wmax, v), wmin = fmin(wmin, v);
                }
            }
            for (int k = tid; k < maxiter; k += NT) {
                const double v = hist[k];
                jmax = fmax(jmax, v), jmin = fmin(jmin, v);
            }
            for (int k = tid; k < P; k += NT) {
                const double v = fit[k];
                jmax = fmax(jmax, v), jmin = fmin(jmin, v);
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                wmax = fmax(wmax, __shfl_xor(wmax, off, kWave)), wmin = fmin(wmin, __shfl_xor(wmin, off, kWave));
                jmax = fmax(jmax, __shfl_xor(jmax, off, kWave)), jmin = fmin(jmin, __shfl_xor(jmin, off, kWave));
            }
            if (lane == 0) {
                part[wave * kPartWords + 0] = wmax, part[wave * kPartWords + 1] = wmin;
                part[wave * kPartWords + 2] = jmax, part[wave * kPartWords + 3] = jmin;
            }
        }
        __syncthreads();
        double wmax = part[0], wmin = part[1], jmax = part[2], jmin = part[3];
#pragma unroll
        for (int w = 1; w < NW; ++w) {
            wmax = fmax(wmax, part[w * kPartWords + 0]), wmin = fmin(wmin, part[w * kPartWords + 1]);
            jmax = fmax(jmax, part[w * kPartWords + 2]), jmin = fmin(jmin, part[w * kPartWords + 3]);
        }
        // per-dimension quantities: lane e of EVERY wavefront takes element e (n <= 32), a butterfly gives every lane of
        // every wavefront the same totals
        const int axis = gen % n;
        const double dax = D[axis];
        double dx2 = 0.0, fail4 = 0.0, any5 = 0.0, dmax = -__builtin_inf(), dmin = __builtin_inf(), any8 = 0.0;
        double sdmax = -__builtin_inf(), fail10 = 0.0, nan_sd = 0.0, nan_d = 0.0;
        const double insigma = kInsigmaAtEntry ? insigma_entry : run_setting(sw.sigma, run, a.insigma);
        if (lane < n) {
            const int e = lane;
            const double d = xold[e] - xmean[e];
            dx2 = d * d;
            if (!(fabs(0.1 * sigma * B[e * ldn + axis] * dax) < 1.0e-10)) fail4 = 1.0;
            const double sd = sqrt(C[e * ldn + e]);
            if (0.2 * sigma * sd < 1.0e-10) any5 = 1.0;
            const double de = D[e];
            dmax = fmax(dmax, de), dmin = fmin(dmin, de);  // (numpy's max/min propagate NaN; rule 6 then compares False either way)
            if (de != de) nan_d = 1.0;
            if (sigma * sd > 1.0e3 * insigma) any8 = 1.0;
            if (sd != sd) nan_sd = 1.0;
            sdmax = fmax(sdmax, sd);
            if (!(sigma * fabs(pc[e]) < 1.0e-11 * insigma)) fail10 = 1.0;
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            dx2 += __shfl_xor(dx2, off, kWave), fail4 += __shfl_xor(fail4, off, kWave), any5 += __shfl_xor(any5, off, kWave);
            any8 += __shfl_xor(any8, off, kWave), fail10 += __shfl_xor(fail10, off, kWave);
            nan_sd += __shfl_xor(nan_sd, off, kWave), nan_d += __shfl_xor(nan_d, off, kWave);
            dmax = fmax(dmax, __shfl_xor(dmax, off, kWave)), sdmax = fmax(sdmax, __shfl_xor(sdmax, off, kWave));
            dmin = fmin(dmin, __shfl_xor(dmin, off, kWave));
        }
        int status = SX_STATUS_NONE;  // cma_stop_status, statement for statement
        if (gen >= maxiter)
            status = -1;
        else if (sqrt(dx2) <= a.xtol && fbest < a.ftol)
            status = 0;
        else if (fbest <= a.ftol)
            status = 1;
        else if (fail4 == 0.0)
            status = -2;
        else if (any5 > 0.0)
            status = -3;
        else if (nan_d == 0.0 && dmax > 1.0e7 * dmin)
            status = -4;
        else if (gen >= a.ilim && wmax - wmin < 1.0e-10)
            status = -5;
        else if (any8 > 0.0)
            status = -6;
        else if (gen > 2 && jmax - jmin < 1.0e-12)
            status = -7;
        else if (fail10 == 0.0 && nan_sd == 0.0 && sigma * sdmax < 1.0e-11 * insigma)
            status = -8;
        if (status != SX_STATUS_NONE) {  // (uniform) the run is over; the other runs' workgroups know nothing of it
            // the caller's result: best candidate of THIS generation, un-standardised (:345-353)
            for (int e = tid; e < n; e += NT) {
                a.xs[run * n + e] = xbest[e] * a.xstd[e] + a.xm[e];
                if (a.xmeans != nullptr) a.xmeans[run * n + e] = xmean[e];
            }
            if (tid == 0) {
                a.funs[run] = fbest;
                a.nits[run] = gen;
                a.statuses[run] = status;
                if (a.nfevs != nullptr) a.nfevs[run] = (int64_t)gen * P;
                if (a.sigmas != nullptr) a.sigmas[run] = sigma;
            }
            return;
        }
        __syncthreads();  // the rules have read fit[], B, C, D: the next generation may write
    }
}

}  // namespace

extern "C" int64_t sx_cma_runs_lds_bytes(int64_t P, int n) {
    if (P < 2 || P > kLdsLimit || n < 1 || n > kRunsMaxDim) return -1;
    const int64_t bytes = (int64_t)runs_layout(P, n).total * (int64_t)sizeof(double);
    return bytes <= kLdsLimit ? bytes : -1;
}

extern "C" int64_t sx_cma_runs_workspace_bytes(int64_t R, int64_t maxiter) { return sigma_runs_workspace_bytes(R, maxiter); }

extern "C" int sx_cma_runs_sweep_launch(const sx_cma_runs_args *a, const double *sigma, void *stream) {
    SX_REQUIRE(a != nullptr, "sx_cma_runs_launch: null args");
    const int64_t lds = sx_cma_runs_lds_bytes(a->P, a->n);
    PlanArg plan;
    if (int rc = prepare_sigma_runs("sx_cma_runs_launch", a, 1, kRunsMaxDim, lds,
                                    "sx_cma_runs_launch: the run's model and candidates do not fit one workgroup's LDS", &plan, stream))
        return rc;
    const SigmaSweep sweep = {sigma};
    if (runs_m2(a->n) == 16) {
        SX_DISPATCH_FUN(a->fun_id,
                        return enqueue_runs(cma_runs_kernel<FUN, 16>, *a, plan, sweep, runs_threads<16>(), lds, stream))
    }
    SX_DISPATCH_FUN(a->fun_id, return enqueue_runs(cma_runs_kernel<FUN, 32>, *a, plan, sweep, runs_threads<32>(), lds, stream))
    return -1;
}

extern "C" int sx_cma_runs_launch(const sx_cma_runs_args *a, void *stream) {
    return sx_cma_runs_sweep_launch(a, nullptr, stream);
}
