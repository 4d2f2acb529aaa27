// The one-workgroup symmetric eigensolver of small matrices (n <= 64: M2 = 16 / 32 / 64): cyclic two-sided Jacobi in LDS.
// Shared by eigh_small_kernel (sx_eigh.hip: one decomposition per launch) and the resident CMA-ES runs (sx_cma_runs.hip: a
// decomposition inside a run's workgroup, whenever the run's own rule says one is due) -- one sweep, so the same rotations.
// eigh_small_kernel keeps its own copy of the few statements that drive the sweeps (eigh_small_sweeps below): written
// against this function it compiled to other instructions.
//
// Reference code replaced (paths relative to the reference checkout):
//   stochopy/optimize/cmaes/_cmaes.py:303-305   D, B = np.linalg.eigh(C) (the sweeps; order and signs are the callers')
#pragma once
#include "sx_device.hpp"

// (sx_eigh.hip's debug build stamps the shader clock inside the sweep: tools/trace_eigh.py)
#ifndef SX_ETQ
#define SX_ETQ(cond, k) do {} while (0)
#endif

// (unnamed namespace at file scope, as sx_eigh.hip had these: the kernels that use them keep their symbol names)
namespace {

constexpr int kEighMaxSweeps = 60;

// Jacobi rotation J = [[c, s], [-s, c]] on the (p,q) plane that (nearly) annihilates a_pq, |angle| <= pi/4.
// With d = a_qq - a_pp, h = 2 a_pq, r = hypot(d, h):  cos 2phi = |d| / r,  sin 2phi = sign(d) h / r,
// c = sqrt((1 + cos 2phi) / 2),  s = sin 2phi / (2 c).  The ANGLE is worked out in single precision (two
// v_rsq_f32, no division, no fp64 square root: this sits on the critical path of every inner round), then
// (c, s) is renormalised in fp64 so that c^2 + s^2 = 1 to rounding: the transform is orthogonal to fp64
// accuracy, and an angle that is off by 1e-7 relative only leaves 1e-7 of a_pq behind (every update below
// applies the rotation that was actually chosen, nothing assumes an exact zero), which the quadratic
// convergence of the sweeps absorbs.
__device__ __forceinline__ void rotation(double app, double aqq, double apq, double &c, double &s) {
    double d = aqq - app, h = 2.0 * apq;
    const double mx = fmax(fabs(d), fabs(h));
    if (h == 0.0 || !(mx < __builtin_inf())) {  // nothing to annihilate (or non-finite input: leave it alone)
        c = 1.0, s = 0.0;
        return;
    }
    int ex;
    (void)frexp(mx, &ex);
    const float df = (float)ldexp(d, -ex), hf = (float)ldexp(h, -ex);  // max(|d|, |h|) in [0.5, 1)
    const float ir = __builtin_amdgcn_rsqf(fmaf(df, df, hf * hf));
    const float x2 = fmaf(0.5f, fabsf(df) * ir, 0.5f);  // c^2 in [0.5, 1]
    const float ic = __builtin_amdgcn_rsqf(x2);
    const double cd = (double)(x2 * ic);
    const double sd = (double)((0.5f * ((df < 0.0f ? -hf : hf) * ir)) * ic);
    const double e = fma(-cd, cd, fma(-sd, sd, 1.0));  // 1 - (c^2 + s^2) ~ 1e-7
    const double k = fma(e, fma(0.375, e, 0.5), 1.0);  // (1 - e)^(-1/2) to e^3
    c = cd * k, s = sd * k;
}

// the LDS arrays one Jacobi sweep works on (the callers own the storage; everything is double-buffered)
struct JacobiView {
    double *S0, *S1;  // [M2][M2 + 1] each: the matrix
    double *W0, *W1;  // [M2][M2 + 1] each: accumulated rotations (rows fixed, columns move with the matrix)
    double *c, *s;    // [2][M2 / 2] rotation of every pair of the current / next inner round
};

// The sweep is systolic: position pair k is ALWAYS (2k, 2k+1), and after every round rows and columns move by
// a fixed permutation, so every thread reads and writes at addresses that never change (no index arithmetic
// inside the loop) and after the last round everything is back in place.
//   MODE 0 (all pairs; M2-1 rounds): the round-robin tournament -- position 0 stays, the other M2-1 rotate by one
//          place: 1 -> 2 -> 4 -> ... -> M2-2 -> M2-1 -> M2-3 -> ... -> 3 -> 1.
//   MODE 1 (only pairs (even, odd) position = (block I, block J) of the outer method; M2/2 rounds): even
//          positions stay, odd positions move on by one pair.
template <int MODE>
__host__ __device__ constexpr int sys_perm(int x, int m) {
    if (MODE == 1) return (x & 1) ? (x + 2 >= m ? 1 : x + 2) : x;
    return x == 0 ? 0 : (x == 1 ? 2 : ((x & 1) ? x - 2 : (x == m - 2 ? m - 1 : x + 2)));
}
template <int MODE>
__host__ __device__ constexpr int sys_perm_inv(int y, int m) {
    if (MODE == 1) return (y & 1) ? (y == 1 ? m - 1 : y - 2) : y;
    return y == 0 ? 0 : (y == 2 ? 1 : ((y & 1) ? (y == m - 1 ? m - 2 : y + 2) : y - 2));
}
template <int M2>
constexpr int jacobi_threads() {  // NP*NP updating threads, plus one wave that only prepares the next rotations
    return (M2 / 2) * (M2 / 2) + 64 <= 1024 ? (M2 / 2) * (M2 / 2) + 64 : (M2 / 2) * (M2 / 2);
}

// one cyclic sweep on the M2 x M2 matrix in S0 (cur = 0) / S1; W <- W J for every rotation.
// One barrier per inner round: while the NP*NP updating threads apply the rotations of round r to their 2x2
// blocks (writing to the permuted places of the other buffer), NP rotation lanes -- a wave of their own when
// the workgroup has room for one -- work out the pivot of their pair of round r+1 from the OLD matrix and the
// rotations of round r, and from it the next rotation.
template <int M2, int MODE>
__device__ void jacobi_sweep(const JacobiView &L, int &cur, const int tid) {
    constexpr int NP = M2 / 2, LD = M2 + 1, NREG = NP * NP, ROUNDS = MODE == 1 ? NP : M2 - 1;
    constexpr bool OWN_WAVE = jacobi_threads<M2>() > NREG;
    const bool reg = tid < NREG;
    const int kp = reg ? tid / NP : 0, kq = reg ? tid % NP : 0;
    // updating threads: source block (2kp, 2kp+1) x (2kq, 2kq+1), destination at the permuted places
    const int o00 = (2 * kp) * LD + 2 * kq, o10 = o00 + LD;
    const int dr0 = sys_perm<MODE>(2 * kp, M2) * LD, dr1 = sys_perm<MODE>(2 * kp + 1, M2) * LD;
    const int dc0 = sys_perm<MODE>(2 * kq, M2), dc1 = sys_perm<MODE>(2 * kq + 1, M2);
    // Rotation lanes.  With a wave of their own (OWN_WAVE) FOUR lanes serve pair k of the next round -- its old
    // positions (i, j) = perm^-1(2k, 2k+1) -- and work out one pivot element each (lane 0: (i,i), 1: (j,j), 2 and 3:
    // (i,j)) with the very operations the updating threads apply, so the predicted pivot IS the next matrix's; a DPP
    // quad broadcast collects the three values and every lane forms the rotation (lane 0 of the quad stores it).
    // Without room for an extra wave (M2 = 64) lane k of wave 0 does the three elements one after the other.
    const int dl = OWN_WAVE ? tid - NREG : tid;
    const bool duty = dl >= 0 && dl < (OWN_WAVE ? 4 * NP : NP);
    const int k2 = duty ? (OWN_WAVE ? dl >> 2 : dl) : 0, part = OWN_WAVE ? (dl & 3) : 0;
    const int i = sys_perm_inv<MODE>(2 * k2, M2), j = sys_perm_inv<MODE>(2 * k2 + 1, M2);
    // element (ea, eb) this lane predicts
    const int ea = part == 1 ? j : i, eb = part == 0 ? i : j;
    const int ka = ea >> 1, kb = eb >> 1;
    const bool pa = ea & 1, pb = eb & 1;
    const int qab = (2 * ka) * LD + 2 * kb;
    auto predicted = [&](const double *S, const double *rc, const double *rs, int ka_, bool pa_, int kb_, bool pb_, int q_) {
        const double ca = rc[ka_], sa = rs[ka_], cb = rc[kb_], sb = rs[kb_];
        const double b00 = S[q_], b01 = S[q_ + 1], b10 = S[q_ + LD], b11 = S[q_ + LD + 1];
        const double r0 = pa_ ? fma(sa, b00, ca * b10) : fma(ca, b00, -(sa * b10));
        const double r1 = pa_ ? fma(sa, b01, ca * b11) : fma(ca, b01, -(sa * b11));
        return pb_ ? fma(sb, r0, cb * r1) : fma(cb, r0, -(sb * r1));
    };
    if (duty) {
        const double *S = cur ? L.S1 : L.S0;
        const int o = (2 * k2) * LD + 2 * k2;
        double c, s;
        rotation(S[o], S[o + LD + 1], S[o + 1], c, s);
        if (part == 0) L.c[k2] = c, L.s[k2] = s;
    }
    __syncthreads();
    for (int r = 0; r < ROUNDS; ++r) {
        const double *S = cur ? L.S1 : L.S0;
        double *Sn = cur ? L.S0 : L.S1;
        const double *W = cur ? L.W1 : L.W0;
        double *Wn = cur ? L.W0 : L.W1;
        const double *rc = L.c + (r & 1) * NP, *rs = L.s + (r & 1) * NP;
        SX_ETQ(r == 5 && tid == 0, 6);
        SX_ETQ(r == 5 && duty && dl == 0, 10);
        if (duty && r + 1 < ROUNDS) {
            double nii, njj, nij;
            if (OWN_WAVE) {
                const double v = predicted(S, rc, rs, ka, pa, kb, pb, qab);
                nii = sx::dpp_f64<0x00>(v);  // quad_perm:[0,0,0,0]
                njj = sx::dpp_f64<0x55>(v);  // quad_perm:[1,1,1,1]
                nij = sx::dpp_f64<0xAA>(v);  // quad_perm:[2,2,2,2]
            } else {
                const int ki = i >> 1, kj = j >> 1;
                const bool pi = i & 1, pj = j & 1;
                nii = predicted(S, rc, rs, ki, pi, ki, pi, (2 * ki) * LD + 2 * ki);
                njj = predicted(S, rc, rs, kj, pj, kj, pj, (2 * kj) * LD + 2 * kj);
                nij = predicted(S, rc, rs, ki, pi, kj, pj, (2 * ki) * LD + 2 * kj);
            }
            SX_ETQ(r == 5 && dl == 0 && nij != 12345.0, 11);
            double c, s;
            rotation(nii, njj, nij, c, s);
            SX_ETQ(r == 5 && dl == 0 && c != 12345.0, 12);
            if (part == 0) L.c[((r + 1) & 1) * NP + k2] = c, L.s[((r + 1) & 1) * NP + k2] = s;
        }
        if (reg) {
            const double c1 = rc[kp], s1 = rs[kp], c2 = rc[kq], s2 = rs[kq];
            const double b00 = S[o00], b01 = S[o00 + 1], b10 = S[o10], b11 = S[o10 + 1];
            const double w00 = W[o00], w01 = W[o00 + 1], w10 = W[o10], w11 = W[o10 + 1];
            // rows: J^T B;  columns: (J^T B) J
            const double r00 = fma(c1, b00, -(s1 * b10)), r01 = fma(c1, b01, -(s1 * b11));
            const double r10 = fma(s1, b00, c1 * b10), r11 = fma(s1, b01, c1 * b11);
            Sn[dr0 + dc0] = fma(c2, r00, -(s2 * r01));
            Sn[dr0 + dc1] = fma(s2, r00, c2 * r01);
            Sn[dr1 + dc0] = fma(c2, r10, -(s2 * r11));
            Sn[dr1 + dc1] = fma(s2, r10, c2 * r11);
            // W <- W J: rows 2kp, 2kp+1 (rows of W stay), columns (2kq, 2kq+1) move like the matrix's
            Wn[(2 * kp) * LD + dc0] = fma(c2, w00, -(s2 * w01));
            Wn[(2 * kp) * LD + dc1] = fma(s2, w00, c2 * w01);
            Wn[(2 * kp + 1) * LD + dc0] = fma(c2, w10, -(s2 * w11));
            Wn[(2 * kp + 1) * LD + dc1] = fma(s2, w10, c2 * w11);
        }
        SX_ETQ(r == 5 && tid == 0, 7);
        SX_ETQ(r == 5 && duty && dl == 0, 13);
        __syncthreads();
        SX_ETQ(r == 5 && tid == 0, 8);
        SX_ETQ(r == 5 && duty && dl == 0, 14);
        cur ^= 1;
    }
}

// sum over the workgroup (all threads get the result); NT threads, fixed order
template <int NT>
__device__ double block_sum(double v, double *red, int tid) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, sx::kWave);
    constexpr int NW = (NT + 63) / 64;
    static_assert(NW <= 17, "red[] holds 17 partial sums");
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < NW; ++w) s += red[w];
    return s;
}

// The sweeps of a decomposition whose caller has put the matrix (upper triangle mirrored, padded with zeros to M2 x M2)
// into S[0] and the identity into W[0] (S, W: [2][M2 * (M2 + 1)] doubles of LDS each, row stride M2 + 1; L: the view of
// the same storage plus the rotations' 2 * M2 doubles; sred: 17 doubles) and hands in its threads' partial sums n2 of
// the squared elements: sweeps until the off-diagonal mass -- measured exactly before every sweep -- is below
// tol * |C|_F, or `max_sweeps` of them.  Called by ALL NT >= jacobi_threads<M2>() threads of the workgroup (the sweep
// contains barriers).  rec(sw, off2): what the caller keeps of the measurement before sweep sw (every thread calls it).
// Afterwards M = V^T C V is in S[cur] and V in W[cur], visible to all threads; n2 = |C|_F^2, thr2 the threshold, sw the
// sweeps carried out, conv whether the rule held.
template <int M2, int NT, class Rec>
__device__ __forceinline__ void eigh_small_sweeps(const JacobiView &L, const double *S, double *sred, int max_sweeps,
                                                  double tol, int tid, int &cur, int &sw, int &conv, double &n2,
                                                  double &thr2, Rec rec) {
    constexpr int LD = M2 + 1;
    static_assert(NT >= jacobi_threads<M2>(), "every updating thread and the rotation wave");
    n2 = block_sum<NT>(n2, sred, tid);
    thr2 = tol * tol * n2;
    cur = 0, sw = 0, conv = 0;
    for (;;) {  // the off-diagonal mass is measured exactly before every sweep: stop as soon as it is below tol
        double off2 = 0.0;
        for (int e = tid; e < M2 * M2; e += NT) {
            const int i = e / M2, j = e % M2;
            const double v = S[cur * (M2 * LD) + i * LD + j];
            if (i != j) off2 += v * v;
        }
        off2 = block_sum<NT>(off2, sred, tid);
        rec(sw, off2);
        if (off2 <= thr2) {
            conv = 1;
            break;
        }
        if (sw >= max_sweeps) break;
        jacobi_sweep<M2, 0>(L, cur, tid);
        ++sw;
    }
}

}  // namespace
