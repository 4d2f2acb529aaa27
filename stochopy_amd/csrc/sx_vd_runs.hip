// Many independent VD-CMA runs in one launch: one workgroup per run, resident from the first generation to the run's own
// stopping rule (include/stochopy_hip.h, sx_vd_runs_args).  A single run at the reference's small populations (10 ... 30
// rows) is six to eight launches per generation, each a fraction of one workgroup; R such runs under R seeds fill the device
// instead.  The model D (I + v v^T) D is O(n): there is no decomposition in the loop, and a run of hundreds of variables
// fits one workgroup's LDS.
//
// Reference code replaced (paths relative to the reference checkout), R times over:
//   stochopy/optimize/vdcma/_vdcma.py:232-425   the generation loop: candidates and injection (:236-248), ranking and mean
//                                               shift (:289-295), rank-gap step size (:298-306), path and model constants
//                                               (:309-328), moments (:331-345, :428-444), natural gradient and the update of
//                                               v and d (:348-378, :447-460)
//   stochopy/optimize/cmaes/_cmaes.py:360-434   converge as vdcma calls it (no B, D: rules -2 and -4 drop out)
//
// RESIDENCY.  Neither the candidates x[P][n] nor the steps y[P][n] exist.  A row's normals are a pure function of
// (slot, row, generation, key) -- cma_normal_pair -- so a step is FORMED AGAIN wherever it is needed, by the expression that
// formed it the first time from the same operands (the same bits; the wide single run re-forms x from y the same way,
// sx_vd_args.arx == NULL):
//   pass 1 (one row per row group of LPR lanes, RPP = NT / LPR rows at a time): z into the group's staging row, t = z . vn,
//           y = d o (z + coef (t vn)), x = xmean + sigma y, the objective of the un-standardised x in that staging row;
//           kept per row: fit, t, and t_k = (y / d) . vn (what the moments want) -- three doubles;
//   pass 2 (after the ranking; one thread per Philox call = pair of elements, G slices of the mu selected rows): y and x of
//           the selected rows again, their weighted sums wx, wy and moments p_mu, q_mu; the first selected row (the best) is
//           written to xbest on the way.  mu <= P / 2 rows cost their normals twice: 1.5 x the draws, no P x n array.
// LDS of a run (doubles; NT = 256 threads for n <= 128, else 512; LPR = lanes_per_row(n), RPP = NT / LPR,
// S = gen_row_stride(n), npair = ceil(n / (2 LPR)) LPR, G = min(8, max(1, NT / npair))), in this order:
//   xmean[n] xold[n] dx[n] d[n] v[n] vn[n] pc[n] dy[n] xbest[n] p[n] q[n] | fit[P] tz[P] tk[P] |
//   order[P] as int32, (P + 1) / 2 doubles | red[80]: the reductions' per-wave partials | pos[8]: ranks of rows 0 and 1 |
//   U = max(RPP S, 8 G npair): the staging rows of pass 1, then (they are dead) the G slices' partial sums of pass 2,
//   part[4][G][2 npair]
// = 11 n + 3 P + (P + 1) / 2 + 88 + max(RPP S, 8 G npair) doubles (sx_vd_runs_lds_bytes).  popsize 10 fits for every
// n <= 512 (78.7 KiB at n = 512), popsize 4 + floor(3 ln n) for every n <= 256; the largest n at P = 10 is 1052.
// The best-fitness history (besthist[maxiter], read by stopping rules -5 and -7) is the run's slice of the caller's
// workspace, zeroed by sx_vd_runs_launch: entry `gen` is read before it is written, as in the reference.
//
// A GENERATION mirrors sx_vdcma_generation (sx_vd_loop.hip, sx_cmaes.hip) with workgroup barriers where it has launches:
// the same normals (counter (slot, row within the run, gen, kPurposeCmaNormal), the injection's normals "row P"), the same
// objective (row_objective<FUN, LPR> on the un-standardised row), key_less for the ranking, the expressions of
// vd_inject_kernel / vd_sample_kernel / vd_moments_partial_kernel / vd_update_kernel in their association order
// (-ffp-contract=off).  The reductions (reduce_many) and the stopping rules' facts (rule_facts_add, history_extremes) are
// those of sx_cma_rules.hpp, shared with the single run.
// LEFT APART, on measurement (profiles/cma_rules_refactor_resources.txt and
// cma_rules_refactor_ab.txt): this kernel's own spelling of that header's cma_stop_status, and the ranking by wave votes,
// which stands here and in cma_runs_kernel (sx_cma_runs.hip).  Every instantiation sits at 256 VGPRs or close.  With the
// cascade as a call -- as values, by reference, with early returns -- vd_runs_kernel<5, 64> and <6, 64> went from 84 to 88
// and 92 bytes of scratch per lane.  The votes as a shared function, alone, made three instantiations gain 4 and 8 bytes;
// next to the other calls they cost no register and gave the same bytes, but n = 64 ran 0.2 ... 0.6 % below the parent's
// own spread (without: inside).  A correction to a rule in the header, or to the votes there, is owed here as well.
//
// ORDERS OF SUMMATION.  They depend on n, P and mu only -- never on R, the grid or the neighbours:
//   * over the elements of a row (t, t_k): lane l of the row's LPR lanes adds its elements in the order pass 1 visits them
//     (pairs l, l + LPR, ...: cosine element, then sine element), the LPR sums meet in an xor butterfly (1, 2, ... LPR / 2);
//   * over n (every dot product, norm, max, min of the update and the injection): thread t adds its elements t, t + NT, ...
//     in order, a wavefront's 64 sums meet in an xor butterfly (32 ... 1), the wavefronts' totals are added in order
//     (reduce_many); the injection's |z|^2 goes by pairs (cosine, then sine) the same way;
//   * over the mu selected rows (wx, wy, p_mu, q_mu): slice g adds the rows k = g, g + G, ... in order, the G slices are
//     added in order;
//   * over P and the history (maxima, minima): order is immaterial.
// The single run leaves these orders to its launch geometry (64 slices, four of sixteen), so run r agrees with the single
// run of its key and with the oracle to rounding, not bit for bit; two launches that hold the same run agree bit for bit.
//
// Nothing passes between workgroups: no grid barrier, no spin-wait, no atomics.  Every loop is bounded by maxiter, P, mu
// or n.
#include "sx_cma_rules.hpp"
#include "sx_device.hpp"
#include "sx_host.hpp"
#include "sx_rowops.hpp"
#include "sx_runs.hpp"

using namespace sx;

namespace {

constexpr int kVrMinDim = 6;               // below, the reference's learning rates are <= 0 (cfactor = (n - 5) / 6)
constexpr int kVrVecs = 11, kVrRed = 80, kVrPos = 8, kVrMaxSlices = 8;

__host__ __device__ inline int vr_threads(int n) { return n <= 128 ? 256 : 512; }
__host__ __device__ inline int vr_npair(int n) {
    const int lpr = lanes_per_row(n);
    return ((n + 2 * lpr - 1) / (2 * lpr)) * lpr;
}
__host__ __device__ inline int vr_slices(int n) {
    const int g = vr_threads(n) / vr_npair(n);
    return g < 1 ? 1 : (g > kVrMaxSlices ? kVrMaxSlices : g);
}

struct VrLayout {  // offsets in doubles (see the header comment)
    int64_t vec, fit, order, red, pos, U, total;
};
__host__ __device__ inline VrLayout vr_layout(int64_t P, int n) {
    const int64_t stage = (int64_t)(vr_threads(n) / lanes_per_row(n)) * gen_row_stride(n);
    const int64_t part = 8 * (int64_t)vr_slices(n) * vr_npair(n);
    VrLayout L;
    L.vec = 0;
    L.fit = L.vec + (int64_t)kVrVecs * n;
    L.order = L.fit + 3 * P;
    L.red = L.order + (P + 1) / 2;
    L.pos = L.red + kVrRed;
    L.U = L.pos + kVrPos;
    L.total = L.U + (stage > part ? stage : part);
    return L;
}

// minimum wavefronts per SIMD asked of the compiler: 2, i.e. up to 256 VGPRs.  The floor of 4 of the other runs kernels (128
// VGPRs) leaves these with 452 ... 1 184 bytes of scratch per lane and was measured 23 ... 47 % slower here
#ifndef SX_VD_RUNS_WAVES
#define SX_VD_RUNS_WAVES 2
#endif
template <int FUN, int LPR>
__global__ __launch_bounds__(LPR == 64 ? 512 : 256, SX_VD_RUNS_WAVES) void vd_runs_kernel(const sx_vd_runs_args a, const PlanArg plan,
                                                                                          const SigmaSweep sw) {
    constexpr int NT = LPR == 64 ? 512 : 256, NW = NT / kWave, RPP = NT / LPR;
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int64_t run = blockIdx.x;
    const int n = a.n, P = (int)a.P, mu = a.mu, maxiter = a.maxiter;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, l = tid & (LPR - 1), slot = tid / LPR;
    const int S = gen_row_stride(n), npair = vr_npair(n), G = vr_slices(n), nP = 2 * npair;
    const VrLayout Lo = vr_layout(P, n);
    double *const xmean = lds + Lo.vec, *const xold = xmean + n, *const dx = xold + n, *const dv = dx + n, *const vv = dv + n;
    double *const vn = vv + n, *const pc = vn + n, *const dy = pc + n, *const xbest = dy + n, *const pp = xbest + n;
    double *const qq = pp + n;
    double *const fit = lds + Lo.fit, *const tzv = fit + P, *const tkv = tzv + P;
    int *const order = reinterpret_cast<int *>(lds + Lo.order);
    double *const red = lds + Lo.red;
    int *const pos = reinterpret_cast<int *>(lds + Lo.pos);
    double *const stage = lds + Lo.U, *const part = lds + Lo.U;
    double *const hist = a.work + run * (int64_t)maxiter;  // zeroed by the launch function
    const uint32_t key0 = a.keys[2 * run], key1 = a.keys[2 * run + 1];
    const double cc = a.cc, c1 = a.c1, cmu = a.cmu;
    const double cpc = sqrt(cc * (2.0 - cc) * a.mueff);
    const bool learn = cmu + c1 > 0.0;

    // ---- the model a run starts from (:202-213): d = 1, the caller's direction and mean, path 0
    double nv2 = 0.0;
    for (int e = tid; e < n; e += NT) {
        const double v0 = a.vvec0[run * n + e];
        xmean[e] = a.xmean0[run * n + e], xold[e] = 0.0, dx[e] = 0.0, dv[e] = 1.0, vv[e] = v0, pc[e] = 0.0, dy[e] = 0.0;
        nv2 += v0 * v0;
    }
    for (int t = tid; t < RPP * S; t += NT) stage[t] = 0.0;  // (a row's padding is read, its value never used)
    {
        double r1[1] = {nv2};
        const int k1[1] = {0};
        reduce_many<1, NW>(r1, k1, red);
        nv2 = r1[0];
    }
    double nv = sqrt(nv2), vmax = -__builtin_inf();
    for (int e = tid; e < n; e += NT) {
        const double v1 = vv[e] / nv;
        vn[e] = v1;
        vmax = fmax(vmax, v1 * v1);
    }
    {
        double r1[1] = {vmax};
        const int k1[1] = {1};
        reduce_many<1, NW>(r1, k1, red);
        vmax = r1[0];
    }
    // the run's own initial step size (a sweep's element `run`; rules -6 and -8 then compare with it), else the struct's
    const double insigma = run_setting(sw.sigma, run, a.insigma);
    double sigma = run_setting(sw.sigma, run, a.sigma), ps = 0.0;  // (uniform: every thread works them out from the same reduced values)
    __syncthreads();

    for (int gen = 1; gen <= maxiter; ++gen) {  // (generation maxiter ends with status -1 at the latest)
        const bool inject = gen >= 2;           // from the second generation on (:304-305)
        const double coef = sqrt(1.0 + nv2) - 1.0;
        // ---- the mean-shift injection (:241-247): dy = |z| / sqrt(mnorm) * dx, z = "row P" of the generation's normals
        if (inject) {  // (uniform)
            double s1 = 0.0, s2 = 0.0, s3 = 0.0;
            for (int e = tid; e < n; e += NT) {
                const double ddx = dx[e] / dv[e];
                s1 += ddx * ddx;
                s2 += ddx * vv[e];
            }
            for (int j = tid; j < npair; j += NT) {
                const int lj = j & (LPR - 1), e0 = 2 * (j - lj) + lj, e1 = e0 + LPR;
                if (e0 >= n) continue;
                double z0, z1;
                cma_normal_pair((uint32_t)j, (uint32_t)P, (uint32_t)gen, key0, key1, z0, z1);
                s3 += z0 * z0;
                if (e1 < n) s3 += z1 * z1;
            }
            double v3[3] = {s1, s2, s3};
            const int k3[3] = {0, 0, 0};
            reduce_many<3, NW>(v3, k3, red);
            const double mnorm = v3[0] - v3[1] * v3[1] / (1.0 + nv2);
            const double fac = sqrt(v3[2]) / sqrt(mnorm);
            for (int e = tid; e < n; e += NT) dy[e] = fac * dx[e];
            __syncthreads();
        }

        // ---- pass 1: candidates (:236-248) and their objective, a row per row group; fit, t = z . vn, t_k = (y / d) . vn
        for (int row = slot; row < P; row += RPP) {
            double *U = stage + (size_t)slot * S;
            const bool inj = inject && row < 2;
            const double sgn = row == 0 ? 1.0 : -1.0;
            double t = 0.0;
            if (!inj) {
                for (int j = l; j < npair; j += LPR) {
                    const int e0 = 2 * (j - l) + l, e1 = e0 + LPR;  // the cosine and the sine half of ONE call (slot j)
                    if (e0 >= n) continue;
                    double z0, z1;
                    cma_normal_pair((uint32_t)j, (uint32_t)row, (uint32_t)gen, key0, key1, z0, z1);
                    U[e0] = z0;
                    t += z0 * vn[e0];
                    if (e1 < n) {
                        U[e1] = z1;
                        t += z1 * vn[e1];
                    }
                }
            }
            t = row_sum<LPR>(t);
            double tk = 0.0;
            for (int e = l; e < n; e += LPR) {  // (this lane's own elements: it wrote their normals itself)
                const double de = dv[e], v1 = vn[e];
                const double y = inj ? sgn * dy[e] : de * (U[e] + coef * (t * v1));
                tk += (y / de) * v1;
                const double x = xmean[e] + sigma * y;
                U[e] = x * a.xstd[e] + a.xm[e];  // cmaes/_cmaes.py:171 unstandardize
            }
            tk = row_sum<LPR>(tk);
            const double f = row_objective<FUN, LPR>(U, n, plan, l);
            lds_wave_fence();  // every lane of the row has read the staged point
            if (l == 0) fit[row] = f, tzv[row] = t, tkv[row] = tk;
        }
        __syncthreads();

        // ---- order = argsort(fit) (:289; NaN last, lower index first on ties): cma_rank_kernel's votes, a wavefront ranks
        //      four rows against 64-key chunks (the same loop as in cma_runs_kernel: see the header comment); where rows 0
        //      and 1 (the injected pair) end up
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
                if (lane == u && i0 + u < P) {
                    order[cnt[u]] = i0 + u;
                    if (i0 + u < 2) pos[i0 + u] = cnt[u];
                }
        }
        __syncthreads();
        const int best_row = order[0];
        const double fbest = fit[best_row];
        if (tid == 0) hist[gen - 1] = fbest;
        // ---- step size from the rank gap of the injected pair (:298-306)
        const double sigma0 = sigma;
        bool cond = true;
        if (inject) {
            const double gap = ((double)pos[1] - (double)pos[0]) / ((double)P - 1.0);
            ps = ps + a.cs * (gap - ps);
            sigma = sigma0 * exp(ps / a.ds);
            cond = ps < 0.5;
        }

        // ---- pass 2: the mu selected rows again (slice g: rows k = g, g + G, ...), their weighted sums (:289-295, :317) and
        //      moments under the model (:331-339, :428-444); the best row aside
        const double shrink = nv2 / (1.0 + nv2);
        for (int i = tid; i < G * npair; i += NT) {
            const int g = i / npair, j = i - g * npair;
            const int lj = j & (LPR - 1), e0 = 2 * (j - lj) + lj, e1 = e0 + LPR;
            double awx0 = 0.0, awy0 = 0.0, ap0 = 0.0, aq0 = 0.0, awx1 = 0.0, awy1 = 0.0, ap1 = 0.0, aq1 = 0.0;
            if (e0 < n) {
                const bool in1 = e1 < n;
                const double d0 = dv[e0], u0 = vn[e0], m0 = xmean[e0], j0 = dy[e0];
                const double d1 = in1 ? dv[e1] : 1.0, u1 = in1 ? vn[e1] : 0.0, m1 = in1 ? xmean[e1] : 0.0, j1 = in1 ? dy[e1] : 0.0;
                for (int k = g; k < mu; k += G) {
                    const int row = order[k];
                    const double wk = a.w[k], t = tzv[row], tk = tkv[row];
                    double y0, y1;
                    if (inject && row < 2) {
                        const double sgn = row == 0 ? 1.0 : -1.0;
                        y0 = sgn * j0, y1 = sgn * j1;
                    } else {
                        double z0, z1;
                        cma_normal_pair((uint32_t)j, (uint32_t)row, (uint32_t)gen, key0, key1, z0, z1);
                        y0 = d0 * (z0 + coef * (t * u0)), y1 = d1 * (z1 + coef * (t * u1));
                    }
                    const double x0 = m0 + sigma0 * y0, x1 = m1 + sigma0 * y1;
                    const double yd0 = y0 / d0, yd1 = y1 / d1;
                    awx0 += wk * x0, awx1 += wk * x1;
                    awy0 += wk * y0, awy1 += wk * y1;
                    ap0 += wk * (yd0 * yd0 - shrink * (tk * (yd0 * u0)) - 1.0);
                    ap1 += wk * (yd1 * yd1 - shrink * (tk * (yd1 * u1)) - 1.0);
                    aq0 += wk * (tk * yd0 - (0.5 * (tk * tk + 1.0 + nv2)) * u0);
                    aq1 += wk * (tk * yd1 - (0.5 * (tk * tk + 1.0 + nv2)) * u1);
                    if (k == 0) {  // the best candidate of this generation (the result reads it)
                        xbest[e0] = x0;
                        if (in1) xbest[e1] = x1;
                    }
                }
            }
            double *p0 = part + (size_t)g * nP;
            const size_t plane = (size_t)G * nP;
            p0[e0] = awx0, p0[plane + e0] = awy0, p0[2 * plane + e0] = ap0, p0[3 * plane + e0] = aq0;
            p0[e1] = awx1, p0[plane + e1] = awy1, p0[2 * plane + e1] = ap1, p0[3 * plane + e1] = aq1;
        }
        __syncthreads();

        // ---- model constants (:317-328)
        const double gamma = 1.0 / sqrt(1.0 + nv2);
        double alpha = sqrt(nv2 * nv2 + (1.0 + nv2) / vmax * (2.0 - gamma)) / (2.0 + nv2);
        double beta = 0.0;
        if (alpha < 1.0) {
            const double t2 = 1.0 + 2.0 / nv2;
            beta = (4.0 - (2.0 - gamma) / vmax) / (t2 * t2);
        } else {
            alpha = 1.0;
        }
        const double bsca = 2.0 * (alpha * alpha) - beta;
        const double acoef = bsca + 2.0 * (alpha * alpha);  // avec = 2 - acoef * vn^2
        // ---- mean shift (:292-294), evolution path (:309-314), y = pc / d, t = y . vn, sum of vn^2 invavnn
        double dx2 = 0.0, t = 0.0, svi = 0.0;
        {
            const size_t plane = (size_t)G * nP;
            for (int e = tid; e < n; e += NT) {
                double wx = part[e], wy = part[plane + e], pmu = part[2 * plane + e], qmu = part[3 * plane + e];
                for (int g = 1; g < G; ++g) {
                    const double *pg = part + (size_t)g * nP + e;
                    wx += pg[0], wy += pg[plane], pmu += pg[2 * plane], qmu += pg[3 * plane];
                }
                const double xm0 = xmean[e];
                const double dxe = wx - a.wsum * xm0;
                dx[e] = dxe, xold[e] = xm0, xmean[e] = xm0 + dxe;
                dx2 += dxe * dxe;
                double pce = pc[e] * (1.0 - cc);
                if (cond) pce = pce + cpc * wy;
                pc[e] = pce;
                const double v1 = vn[e], y = pce / dv[e], vnn = v1 * v1;
                t += y * v1;
                svi += vnn * (vnn / (2.0 - acoef * vnn));
                pp[e] = cmu != 0.0 ? cmu * pmu : 0.0;
                qq[e] = cmu != 0.0 ? cmu * qmu : 0.0;
            }
            double v3[3] = {dx2, t, svi};
            const int k3[3] = {0, 0, 0};
            reduce_many<3, NW>(v3, k3, red);
            dx2 = v3[0], t = v3[1], svi = v3[2];
        }
        // ---- moments of the path (:340-345, :428-444), p and q (:348-352), vn . q
        // (from here to the update every element of p, q is read and written by the one thread that owns it)
        double vq = 0.0;
        for (int e = tid; e < n; e += NT) {
            const double v1 = vn[e];
            double p = pp[e], q = qq[e];
            if (cond && c1 != 0.0) {
                const double y = pc[e] / dv[e];
                const double p_one = (y * y - shrink * ((t * y) * v1)) - 1.0;
                const double q_one = t * y - (0.5 * ((t * t + 1.0) + nv2)) * v1;
                p = p + c1 * p_one;
                q = q + c1 * q_one;
                pp[e] = p, qq[e] = q;
            }
            vq += v1 * q;
        }
        {
            double r1[1] = {vq};
            const int k1[1] = {0};
            reduce_many<1, NW>(r1, k1, red);
            vq = r1[0];
        }
        // ---- natural gradient (:447-460)
        double ri = 0.0;
        for (int e = tid; e < n; e += NT) {  // r overwrites p
            const double v1 = vn[e], vnn = v1 * v1;
            const double r = pp[e] - alpha / (1.0 + nv2) * (((2.0 + nv2) * qq[e]) * v1 - (nv2 * vq) * vnn);
            pp[e] = r;
            ri += r * (vnn / (2.0 - acoef * vnn));
        }
        {
            double r1[1] = {ri};
            const int k1[1] = {0};
            reduce_many<1, NW>(r1, k1, red);
            ri = r1[0];
        }
        double svn = 0.0;
        for (int e = tid; e < n; e += NT) {  // s overwrites r
            const double v1 = vn[e], vnn = v1 * v1, av = 2.0 - acoef * vnn;
            const double s = pp[e] / av - bsca * ri / (1.0 + bsca * svi) * (vnn / av);
            pp[e] = s;
            svn += s * vnn;
        }
        {
            double r1[1] = {svn};
            const int k1[1] = {0};
            reduce_many<1, NW>(r1, k1, red);
            svn = r1[0];
        }
        double g2 = 0.0, mind = __builtin_inf();
        for (int e = tid; e < n; e += NT) {  // ngv overwrites q, ngd overwrites s
            double ngv = 0.0, ngd = 0.0;
            if (learn) {
                const double v1 = vn[e], de = dv[e], s = pp[e];
                ngv = qq[e] / nv - alpha / nv * ((2.0 + nv2) * (v1 * s) - svn * v1);
                ngd = de * s;
                g2 += ngv * ngv;
                mind = fmin(mind, de / fabs(ngd));
            }
            qq[e] = ngv, pp[e] = ngd;
        }
        {
            double v2[2] = {g2, mind};
            const int k2[2] = {0, 2};
            reduce_many<2, NW>(v2, k2, red);
            g2 = v2[0], mind = v2[1];
        }
        double up = 1.0;
        if (learn) {
            up = fmin(1.0, 0.7 * nv / sqrt(g2));
            up = fmin(up, 0.7 * mind);
        }
        // ---- update of v and d (:371-378); the stopping rules' per-dimension counts on the model the candidates were drawn
        //      with and the NEW sigma, pc, mean; the best-fitness histories (window [gen - ilim, gen] of the zero-initialised
        //      array, and the whole array joined with this generation's fitness values)
        double nv2n = 0.0, any3 = 0.0, any6 = 0.0, fail8 = 0.0, nan_sd = 0.0, sdmax = -__builtin_inf();
        for (int e = tid; e < n; e += NT) {
            const double de = dv[e], v0 = vv[e];
            const double sd = sqrt((de * (1.0 + v0 * v0)) * de);  // sqrt of diag D (I + v v^T) D (:249-254)
            const double vnew = v0 + up * qq[e];
            vv[e] = vnew;
            dv[e] = de + up * pp[e];
            nv2n += vnew * vnew;
            rule_facts_add(sd, sigma, insigma, pc[e], any3, any6, nan_sd, sdmax, fail8);
        }
        double wmax, wmin, jmax, jmin;
        history_extremes<int>(hist, fit, gen, a.ilim, maxiter, P, tid, NT, wmax, wmin, jmax, jmin);
        {
            double v10[10] = {nv2n, any3, any6, fail8, nan_sd, sdmax, wmax, jmax, wmin, jmin};
            const int k10[10] = {0, 0, 0, 0, 0, 1, 1, 1, 2, 2};
            reduce_many<10, NW>(v10, k10, red);
            nv2n = v10[0], any3 = v10[1], any6 = v10[2], fail8 = v10[3], nan_sd = v10[4], sdmax = v10[5], wmax = v10[6];
            jmax = v10[7], wmin = v10[8], jmin = v10[9];
        }
        int status = SX_STATUS_NONE;  // cma_stop_status without rules -2 and -4, statement for statement (see the header comment)
        if (gen >= maxiter)
            status = -1;
        else if (sqrt(dx2) <= a.xtol && fbest < a.ftol)
            status = 0;
        else if (fbest <= a.ftol)
            status = 1;
        else if (any3 > 0.0)
            status = -3;
        else if (gen >= a.ilim && wmax - wmin < 1.0e-10)
            status = -5;
        else if (any6 > 0.0)
            status = -6;
        else if (gen > 2 && jmax - jmin < 1.0e-12)
            status = -7;
        else if (fail8 == 0.0 && nan_sd == 0.0 && sigma * sdmax < 1.0e-11 * insigma)
            status = -8;
        if (status != SX_STATUS_NONE) {  // (uniform) the run is over; the other runs' workgroups know nothing of it
            // the caller's result: best candidate of THIS generation, un-standardised
            for (int e = tid; e < n; e += NT) {
                a.xs[run * n + e] = xbest[e] * a.xstd[e] + a.xm[e];
                if (a.xmeans != nullptr) a.xmeans[run * n + e] = xmean[e];
                if (a.dvecs != nullptr) a.dvecs[run * n + e] = dv[e];
                if (a.vvecs != nullptr) a.vvecs[run * n + e] = vv[e];
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
        // ---- the model the next generation samples from: |v|^2, |v|, vn = v / |v|, max vn^2
        nv2 = nv2n, nv = sqrt(nv2n);
        double vm = -__builtin_inf();
        for (int e = tid; e < n; e += NT) {
            const double v1 = vv[e] / nv;
            vn[e] = v1;
            vm = fmax(vm, v1 * v1);
        }
        {
            double r1[1] = {vm};
            const int k1[1] = {1};
            reduce_many<1, NW>(r1, k1, red);
            vmax = r1[0];
        }
        __syncthreads();  // the update is complete (and pass 2's partial sums are dead): the next generation may write
    }
}

}  // namespace

extern "C" int sx_vd_runs_args_bytes(void) { return (int)sizeof(sx_vd_runs_args); }

extern "C" int64_t sx_vd_runs_lds_bytes(int64_t P, int n) {
    if (P < 2 || P > kLdsLimit || n < kVrMinDim || n > kWideFrom) return -1;
    const int64_t bytes = vr_layout(P, n).total * (int64_t)sizeof(double);
    return bytes <= kLdsLimit ? bytes : -1;
}

extern "C" int64_t sx_vd_runs_workspace_bytes(int64_t R, int64_t maxiter) { return sigma_runs_workspace_bytes(R, maxiter); }

extern "C" int sx_vd_runs_sweep_launch(const sx_vd_runs_args *a, const double *sigma, void *stream) {
    SX_REQUIRE(a != nullptr, "sx_vd_runs_launch: null args");
    const int64_t lds = sx_vd_runs_lds_bytes(a->P, a->n);
    PlanArg plan;
    SX_REQUIRE(a->vvec0 != nullptr, "sx_vd_runs_launch: null device pointer");
    if (int rc = prepare_sigma_runs("sx_vd_runs_launch", a, kVrMinDim, kWideFrom, lds,
                                    "sx_vd_runs_launch: the run's model and staging rows do not fit one workgroup's LDS", &plan, stream))
        return rc;
    const SigmaSweep sweep = {sigma};
    SX_DISPATCH_LPR(a->n, SX_DISPATCH_FUN(a->fun_id, return enqueue_runs(vd_runs_kernel<FUN, LPR>, *a, plan, sweep,
                                                                         vr_threads(a->n), lds, stream)))
    return -1;
}

extern "C" int sx_vd_runs_launch(const sx_vd_runs_args *a, void *stream) {
    return sx_vd_runs_sweep_launch(a, nullptr, stream);
}
