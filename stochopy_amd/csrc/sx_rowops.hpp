// Row-level device routines shared by the evaluation / DE / PSO kernels:
// row <-> lane indexing, LDS-staged objective evaluation, per-workgroup best.
#pragma once
#include "sx_device.hpp"

namespace sx {

// LPR lanes own one row; a wave carries RPW = 64 / LPR rows.
template <int LPR>
struct RowIds {
    static constexpr int RPW = kWave / LPR;
    int wave, lane;  // wave in workgroup, lane in wave
    int l;           // lane within the row
    int slot;        // row slot within the workgroup
    int block;       // row workgroup index (blockIdx.x minus the leading service workgroups)
    int64_t row, rowc;
    bool active;
    __device__ __forceinline__ explicit RowIds(int64_t P, int first_block = 0) {
        wave = (int)(threadIdx.x >> 6);
        lane = (int)(threadIdx.x & 63);
        l = lane & (LPR - 1);
        slot = wave * RPW + lane / LPR;
        const int rows_in_block = (int)(blockDim.x >> 6) * RPW;
        block = (int)blockIdx.x - first_block;
        row = (int64_t)block * rows_in_block + slot;
        active = row < P;
        rowc = active ? row : P - 1;  // padding rows shadow the last row and store nothing
    }
};

struct Geometry {
    unsigned blocks, threads;
    size_t lds;
};
inline Geometry row_geometry(int64_t P, int n, int wide_from) {
    // wide rows (n > wide_from, sx_wide.hip): one row and one record per workgroup; the kernels that still walk such a row with
    // ONE wavefront (candidate / selection / radius kernels: no staging) are launched with 64 threads and no dynamic LDS
    if (n > wide_from) return Geometry{(unsigned)P, (unsigned)kWave, 0};
    const int wpb = waves_per_block(n);
    const int rpb = rows_per_block(n);
    return Geometry{(unsigned)((P + rpb - 1) / rpb), (unsigned)(wpb * kWave),
                    (size_t)rpb * lds_row_stride(n) * sizeof(double)};
}

// LDS traffic of one wavefront is processed in issue order, so data a lane wrote is
// visible to the other lanes of the SAME wave once the write has been issued; this
// only keeps the compiler from moving LDS accesses across the hand-off.
__device__ __forceinline__ void lds_wave_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// reductions over the LPR lanes of a row (LPR is a power of two, rows are LPR-aligned)
template <int LPR>
__device__ __forceinline__ double row_min(double v) {
#pragma unroll
    for (int off = 1; off < LPR; off <<= 1) v = fmin(v, __shfl_xor(v, off, kWave));
    return v;
}
template <int LPR>
__device__ __forceinline__ double row_sum(double v) {
#pragma unroll
    for (int off = 1; off < LPR; off <<= 1) v += __shfl_xor(v, off, kWave);
    return v;
}

// One-batch rows of 64 / 128 elements (one leaf of numpy's recursion: <= 128 terms), round 4: the objective WITHOUT the
// term arrays.  numpy's sum is eight accumulators r_j = a[j] + a[8+j] + a[16+j] + ... (strictly left to right), the tree
// ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), then the tail terms one by one (loops_utils.h.src pairwise_sum).  Lane
// L = SEG*j + g of the row (SEG = LPR/8 lanes per accumulator) reads the four elements 8(4g+i)+j, i = 0..3, of the staged
// vector, forms their terms in registers and adds them -- in order -- onto the running sum that arrives from lane L-1
// (same quad: one DPP move): accumulator j's chain walks through SEG adjacent lanes and ends in lane SEG*j + SEG-1.
// Same additions in the same order as numpy (same bits) with 2 LDS reads per term and no term array staged in LDS (the
// objective was 0.7 us of the 6.9 us generation at the metric shape).
template <int FUN, int LPR, int NFIX>
__device__ __forceinline__ double row_objective_chain(const double *U, int l) {
    using O = Obj<FUN>;
    constexpr bool TWO = O::TWO, BMUL = O::BMUL;
    // n = 256 with one term per element: numpy splits 256 = 128 + 128, two such leaves -- the row's two 32-lane halves
    constexpr int NLEAF = NFIX > 128 ? 2 : 1;
    constexpr int M = (O::NEXT ? NFIX - 1 : NFIX) / NLEAF;  // terms per leaf
    constexpr int SEG = LPR / kGroup / NLEAF;               // lanes per accumulator chain: 2 (n = 64) or 4 (n = 128, 256)
    static_assert(NFIX == 4 * LPR && (SEG == 2 || SEG == 4) && M <= 128 && (NLEAF == 1 || !O::NEXT),
                  "one leaf (or two full ones), four elements per lane");
    constexpr int NB = M / kGroup, TAIL = M % kGroup;  // blocks that go into the accumulators; tail terms
    static_assert(TAIL == 0 || NB == 4 * SEG - 1, "the tail is the last block");
    constexpr int kHop = SEG == 4 ? 0x90 : 0xA0;  // quad_perm [0,0,1,2] / [0,0,2,2]: lane L takes lane L-1's value
    constexpr int LPL = LPR / NLEAF;               // lanes per leaf
    const int leaf0 = NLEAF == 2 ? (l / LPL) * (NFIX / 2) : 0;  // first element of this lane's leaf
    const int j = (l % LPL) / SEG, g = l % SEG;
    double a[4], b[4];
    {
        double x[4], xn[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = leaf0 + kGroup * (4 * g + i) + j;
            x[i] = U[e];
            xn[i] = O::NEXT ? U[e + 1] : 0.0;  // (U[NFIX .. NFIX+7] is padding: the term of element NFIX-1 is never used)
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) O::term(x[i], xn[i], leaf0 + kGroup * (4 * g + i) + j, a[i], b[i]);
    }
    // the chain: segment s continues from what segment s-1 hands over.  Every lane runs every segment's code; only the
    // lanes whose turn it is (g == s) hold meaningful values, and only those are passed on.
    double ra = a[0], rb = b[0];
#pragma unroll
    for (int i = 1; i < 4; ++i) {
        if (i < NB) {
            ra = ra + a[i];
            if (TWO) rb = combine<BMUL>(rb, b[i]);
        }
    }
#pragma unroll
    for (int s = 1; s < SEG; ++s) {
        ra = dpp_f64<kHop>(ra);
        if (TWO) rb = dpp_f64<kHop>(rb);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (4 * s + i < NB) {
                ra = ra + a[i];
                if (TWO) rb = combine<BMUL>(rb, b[i]);
            }
        }
    }
    // r_j sits in lane SEG*j + SEG-1; the tree over j (each + / * commutes exactly)
    constexpr int kShl1 = 0x100 + SEG, kShl2 = 0x100 + 2 * SEG;  // row_shl: lane L takes lane L+SEG / L+2 SEG
    ra = combine<false>(ra, dpp_f64<kShl1>(ra));
    ra = combine<false>(ra, dpp_f64<kShl2>(ra));
    if (TWO) {
        rb = combine<BMUL>(rb, dpp_f64<kShl1>(rb));
        rb = combine<BMUL>(rb, dpp_f64<kShl2>(rb));
    }
    double sa, sb = BMUL ? 1.0 : 0.0;
    if constexpr (SEG == 2) {  // a row is one 16-lane DPP row: the last level is a DPP move too
        ra = combine<false>(ra, dpp_f64<0x108>(ra));
        if (TWO) rb = combine<BMUL>(rb, dpp_f64<0x108>(rb));
        sa = row_lane_value<LPR>(ra, SEG - 1, l);
        if (TWO) sb = row_lane_value<LPR>(rb, SEG - 1, l);
    } else if constexpr (NLEAF == 1) {  // two DPP rows: (r0..r3) in lane 3, (r4..r7) in lane 19
        sa = row_lane_value<LPR>(ra, SEG - 1, l) + row_lane_value<LPR>(ra, 4 * SEG + SEG - 1, l);
        if (TWO) sb = combine<BMUL>(row_lane_value<LPR>(rb, SEG - 1, l), row_lane_value<LPR>(rb, 4 * SEG + SEG - 1, l));
    } else {  // two leaves: leaf 0 ends in lanes 3 / 19, leaf 1 in lanes 35 / 51; numpy adds leaf 0 + leaf 1
        sa = (row_lane_value<LPR>(ra, 3, l) + row_lane_value<LPR>(ra, 19, l)) +
             (row_lane_value<LPR>(ra, 35, l) + row_lane_value<LPR>(ra, 51, l));
        if (TWO)
            sb = combine<BMUL>(combine<BMUL>(row_lane_value<LPR>(rb, 3, l), row_lane_value<LPR>(rb, 19, l)),
                               combine<BMUL>(row_lane_value<LPR>(rb, 35, l), row_lane_value<LPR>(rb, 51, l)));
    }
    if constexpr (TAIL > 0) {
        // the tail terms a[M-7 .. M-1] are added one by one to the total: every lane forms them itself from TAIL + 1
        // broadcast reads of the staged vector (independent of the chains above, so they hide behind them) instead of
        // fetching them from the lanes that own those elements (4 cross-lane moves per term and stream)
        double tx[TAIL + 1];
#pragma unroll
        for (int t = 0; t <= TAIL; ++t) tx[t] = U[kGroup * NB + t];
#pragma unroll
        for (int t = 0; t < TAIL; ++t) {
            double ta, tb;
            O::term(tx[t], tx[t + 1], kGroup * NB + t, ta, tb);
            sa = sa + ta;
            if (TWO) sb = combine<BMUL>(sb, tb);
        }
    }
    sa = 0.0 + sa;  // add.reduce starts from the identity
    sb = !TWO ? (BMUL ? 1.0 : 0.0) : (BMUL ? sb : 0.0 + sb);
    return O::finish(sa, sb, NFIX);
}

// objectives whose terms are a few multiplications (no cosine): for these the summation plan, not the arithmetic, is the
// row's time, and long rows of the usual lengths get the plan as constants (row_reduce_long)
template <int FUN>
constexpr bool light_objective() {
    return light_objective(FUN);
}
// The same register chains for rows whose length is only known at run time (shapes off the benchmark grid: n = 100, 130,
// 250 ...).  A row that fits one batch (n <= 4 LPR, i.e. EVERY row of up to 256 elements) has at most three leaves in numpy's recursion, each
// of at most 16 blocks, and only the last one has a tail:
//   m <= 128: one leaf;   m in 129..256: split at n2 = (m/2) - (m/2) % 8 -- and the right part r = m - n2 once more if it
//   is still above 128 (129..135: m = 249..255): 64 + (r - 64), two leaves of at most 8 blocks -- S0 + (S1 + S2).
// A leaf of nb blocks from element e0 lives on a group of 8 SEG lanes exactly as in row_objective_chain -- lane SEG j + g forms
// the terms of blocks 4g .. 4g+3 of accumulator j (leaf_terms_rt: every lane at most four terms, whatever the leaf layout), the
// running sum hops from lane to lane by DPP (leaf_chain_rt) -- with the block count as a run-time value: a block beyond it
// contributes nothing.  After leaf_chain_rt lane SEG-1 (SEG = 2: the whole tree) or lanes SEG-1 and 4 SEG + SEG-1 (SEG = 4:
// the two halves of the last tree level) of the group hold the leaf's sums.  Same additions in the same order as numpy.
template <int FUN>
__device__ __forceinline__ void leaf_terms_rt(const double *U, int e0, int nb, int j, int g, double (&a)[4], double (&b)[4]) {
    using O = Obj<FUN>;
    double x[4], xn[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const bool in = 4 * g + i < nb;
        const int e = e0 + kGroup * (4 * g + i) + j;
        x[i] = in ? U[e] : 0.0;
        xn[i] = (O::NEXT && in) ? U[e + 1] : 0.0;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) O::term(x[i], xn[i], e0 + kGroup * (4 * g + i) + j, a[i], b[i]);
}
template <int FUN, int SEG>
__device__ __forceinline__ void leaf_chain_rt(const double (&a)[4], const double (&b)[4], int nb, double &ra, double &rb) {
    using O = Obj<FUN>;
    constexpr bool TWO = O::TWO, BMUL = O::BMUL;
    static_assert(SEG == 2 || SEG == 4, "16 or 32 lanes per leaf");
    constexpr int kHop = SEG == 4 ? 0x90 : 0xA0;  // quad_perm [0,0,1,2] / [0,0,2,2]: lane L takes lane L-1's value
    ra = a[0], rb = b[0];
#pragma unroll
    for (int i = 1; i < 4; ++i) {
        const bool in = i < nb;
        ra = in ? ra + a[i] : ra;
        if (TWO) rb = in ? combine<BMUL>(rb, b[i]) : rb;
    }
#pragma unroll
    for (int s = 1; s < SEG; ++s) {
        ra = dpp_f64<kHop>(ra);
        if (TWO) rb = dpp_f64<kHop>(rb);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const bool in = 4 * s + i < nb;
            ra = in ? ra + a[i] : ra;
            if (TWO) rb = in ? combine<BMUL>(rb, b[i]) : rb;
        }
    }
    constexpr int kShl1 = 0x100 + SEG, kShl2 = 0x100 + 2 * SEG;  // row_shl: lane L takes lane L+SEG / L+2 SEG
    ra = combine<false>(ra, dpp_f64<kShl1>(ra));
    ra = combine<false>(ra, dpp_f64<kShl2>(ra));
    if (TWO) {
        rb = combine<BMUL>(rb, dpp_f64<kShl1>(rb));
        rb = combine<BMUL>(rb, dpp_f64<kShl2>(rb));
    }
    if constexpr (SEG == 2) {  // the group is one 16-lane DPP row: the last level is a DPP move too
        ra = combine<false>(ra, dpp_f64<0x108>(ra));
        if (TWO) rb = combine<BMUL>(rb, dpp_f64<0x108>(rb));
    }
}

template <int FUN, int LPR>
__device__ __forceinline__ double row_objective_chain_rt(const double *U, int n, const PlanArg &plan, int l) {
    using O = Obj<FUN>;
    constexpr bool TWO = O::TWO, BMUL = O::BMUL;
    const double identB = BMUL ? 1.0 : 0.0;
    const int m = O::NEXT ? n - 1 : n;
    const int nbt = m / kGroup, tail = m % kGroup;  // blocks in all leaves together; terms behind the last leaf's tree
    // the tail terms a[8 nbt .. m-1] are added one by one to the last leaf's sum.  Cheap terms: every lane forms them itself from
    // broadcast reads; a cosine per term: lane t of the row forms term t, and the sums below fetch it
    constexpr bool kTailByLane = !light_objective<FUN>() || LPR == kWave;
    double tla = 0.0, tlb = identB;
    if (kTailByLane && tail > 0) {
        const int e = kGroup * nbt + (l < tail ? l : 0);
        O::term(U[e], O::NEXT ? U[e + 1] : 0.0, e, tla, tlb);
    }
    auto add_tail = [&](double &xa, double &xb) {
#pragma unroll
        for (int t = 0; t < kGroup - 1; ++t) {
            if (t < tail) {  // (uniform)
                double ta, tb;
                if constexpr (kTailByLane) {
                    ta = row_lane_value<LPR>(tla, t, l);
                    tb = TWO ? row_lane_value<LPR>(tlb, t, l) : identB;
                } else {
                    const int e = kGroup * nbt + t;
                    O::term(U[e], O::NEXT ? U[e + 1] : 0.0, e, ta, tb);
                }
                xa = xa + ta;
                if (TWO) xb = combine<BMUL>(xb, tb);
            }
        }
    };
    double sa = 0.0, sb = identB;
    double a[4], b[4], ra, rb;
    if constexpr (LPR < kWave) {  // n <= 128: at most one leaf, on all of the row's lanes
        constexpr int SEG = LPR / kGroup;
        leaf_terms_rt<FUN>(U, 0, nbt, l / SEG, l % SEG, a, b);
        leaf_chain_rt<FUN, SEG>(a, b, nbt, ra, rb);
        if (nbt > 0) {
            if constexpr (SEG == 2) {
                sa = row_lane_value<LPR>(ra, SEG - 1, l);
                if (TWO) sb = row_lane_value<LPR>(rb, SEG - 1, l);
            } else {
                sa = row_lane_value<LPR>(ra, SEG - 1, l) + row_lane_value<LPR>(ra, 4 * SEG + SEG - 1, l);
                if (TWO) sb = combine<BMUL>(row_lane_value<LPR>(rb, SEG - 1, l), row_lane_value<LPR>(rb, 4 * SEG + SEG - 1, l));
            }
        }
        add_tail(sa, sb);
    } else {
        // whole-wave rows of up to 256 elements.  One or two leaves: leaf 0 on lanes 0..31, leaf 1 on lanes 32..63 (32 lanes
        // each: SEG = 4).  Three leaves: leaf 0 as before, leaves 1 and 2 (at most 8 blocks each) on lanes 32..47 and 48..63
        // (16 lanes each: SEG = 2).  Terms are formed ONCE, four per lane; with three leaves both chain forms run over them and
        // each half of the wave keeps the one that is its own.
        const int nleaf = plan.nleaf;  // 0 (m < 8), 1, 2 or 3
        const int end0 = nleaf > 0 ? plan.end[0] : 0, end1 = nleaf > 1 ? plan.end[1] : end0;
        const bool three = nleaf > 2;  // (uniform)
        const int half = l >> 5;
        const bool narrow = three && half;  // this lane belongs to a 16-lane group
        const int lg = narrow ? (l & 15) : (l & 31), grp = (l >> 4) & 1;
        const int seg = narrow ? 2 : 4;
        const int e0 = kGroup * (!half ? 0 : !three ? end0 : grp ? end1 : end0);
        const int nb = !half ? end0 : !three ? end1 - end0 : grp ? nbt - end1 : end1 - end0;
        leaf_terms_rt<FUN>(U, e0, nb, lg / seg, lg % seg, a, b);
        leaf_chain_rt<FUN, 4>(a, b, nb, ra, rb);
        const double s0a = readlane_f64(ra, 3) + readlane_f64(ra, 19);
        double s1a = readlane_f64(ra, 35) + readlane_f64(ra, 51), s2a = 0.0;
        double s0b = identB, s1b = identB, s2b = identB;
        if (TWO) {
            s0b = combine<BMUL>(readlane_f64(rb, 3), readlane_f64(rb, 19));
            s1b = combine<BMUL>(readlane_f64(rb, 35), readlane_f64(rb, 51));
        }
        if (three) {  // (uniform)
            leaf_chain_rt<FUN, 2>(a, b, nb, ra, rb);
            s1a = readlane_f64(ra, 33), s2a = readlane_f64(ra, 49);
            if (TWO) s1b = readlane_f64(rb, 33), s2b = readlane_f64(rb, 49);
        }
        // the last leaf takes the tail before the merges
        double la = three ? s2a : nleaf > 1 ? s1a : s0a, lb = three ? s2b : nleaf > 1 ? s1b : s0b;
        if (nleaf == 0) la = 0.0, lb = identB;
        add_tail(la, lb);
        // merges in recursion order: S0 + S1, or S0 + (S1 + S2)
        if (three) {
            sa = s0a + (s1a + la);
            if (TWO) sb = combine<BMUL>(s0b, combine<BMUL>(s1b, lb));
        } else if (nleaf > 1) {
            sa = s0a + la;
            if (TWO) sb = combine<BMUL>(s0b, lb);
        } else {
            sa = la, sb = lb;
        }
    }
    sa = 0.0 + sa;  // add.reduce starts from the identity
    sb = !TWO ? identB : (BMUL ? sb : 0.0 + sb);
    return O::finish(sa, sb, n);
}

// rows whose objective is the compile-time register chain (row_objective_chain): whole-batch rows of 64 / 128 elements, and of
// 256 with one term per element (two full leaves)
template <int FUN, int NFIX>
constexpr bool chain_only() {
    return NFIX != 0 && (NFIX <= 128 || (NFIX == 256 && !Obj<FUN>::NEXT));
}

// Objective of the row staged in LDS at U[0..n): the terms are formed from the staged vector inside the numpy-order row sum,
// nothing else is staged (whole-wave rows of more than 256 elements keep their leaf sums behind U[n + 8]).
// Every lane of the row returns the value.  Each row works on its own LDS slice (no workgroup barrier).
// NFIX: the row length when it is a compile-time constant (the PSO kernel's whole-batch rows), else 0
// LONGSTATIC = 0: no branch to the compile-time plans of n = 512 / 1024 / 2048 (the one-workgroup kernels of
// updating="immediate", 1 024 threads at the 128-VGPR cap, would spill for them)
// ONEBATCH: the caller guarantees n <= 4 LPR (a whole-wave kernel instantiated for rows of up to 256 elements): nothing but the
// run-time register chain is compiled (the kernel then does not carry the long rows' plans in its register budget)
template <int FUN, int LPR, int NFIX = 0, int LONGSTATIC = 1, bool ONEBATCH = false>
__device__ __forceinline__ double row_objective(double *U, int n, const PlanArg &plan, int l) {
    using O = Obj<FUN>;
    lds_wave_fence();  // U complete (written and read by this wave only)
    if constexpr (chain_only<FUN, NFIX>()) {
        return row_objective_chain<FUN, LPR, NFIX>(U, l);
    } else if constexpr (LPR < kWave || ONEBATCH || (NFIX != 0 && NFIX <= 256)) {
        // one-batch rows (every n <= 256) without a compile-time chain form: the same chains, run-time block counts.
        // (lanes_per_row gives 16 / 32 lanes to rows of up to 64 / 128 elements only: a short-row kernel never meets a longer
        //  row.  NFIX = 256 with an objective that reads the next element -- m = 255: three leaves -- comes here too.)
        return row_objective_chain_rt<FUN, LPR>(U, n, plan, l);
    } else if constexpr (NFIX > 256) {  // a long row of compile-time length: numpy's plan as constants (row_reduce_long)
        double sa, sb;
        row_reduce_long<FUN, (O::NEXT ? NFIX - 1 : NFIX), (light_objective<FUN>() ? 8 : 4)>(U, l, sa, sb);
        return O::finish(sa, sb, NFIX);
    } else {  // a whole-wave row of run-time length
        if (n <= 4 * LPR) return row_objective_chain_rt<FUN, LPR>(U, n, plan, l);
        if constexpr (LONGSTATIC != 0 && light_objective<FUN>()) {
            // long rows of the usual lengths inside the generation kernels (BASELINE config 5: n = 1024): the same constants,
            // picked by a uniform branch on the run-time length
            if (n == 1024 || n == 512 || n == 2048) {
                double sa, sb;
                if (n == 1024)
                    row_reduce_long<FUN, (O::NEXT ? 1023 : 1024)>(U, l, sa, sb);
                else if (n == 512)
                    row_reduce_long<FUN, (O::NEXT ? 511 : 512)>(U, l, sa, sb);
                else
                    row_reduce_long<FUN, (O::NEXT ? 2047 : 2048)>(U, l, sa, sb);
                return O::finish(sa, sb, n);
            }
        }
        double sa, sb;  // terms are formed inside the reduction; the leaf sums sit behind the vector
        row_reduce_leaves_fused<FUN, LPR>(U, U + n + 8, leaf_cap(n), plan, l, sa, sb);
        return O::finish(sa, sb, n);
    }
}

// one (min f, first row) record per workgroup for the best-of-generation step
template <int LPR>
__device__ __forceinline__ void block_partial(double val, const RowIds<LPR> &id, double *sf, int64_t *si,
                                              double *__restrict__ part_f, int64_t *__restrict__ part_i) {
    if (id.l == 0) {
        sf[id.slot] = id.active ? val : __builtin_huge_val();
        si[id.slot] = id.active ? id.row : INT64_MAX;
    }
    __syncthreads();
    // wavefront 0 takes slot k in lane k (slots are in row order) and finds the record with one DPP minimum + ballot.
    // (One lane folding the slots in a 15-step compare-and-select chain cost 0.8 us at the end of every workgroup of
    // the metric shape -- 8.4 -> 7.6 us per generation.)
    if (threadIdx.x < kWave) {
        const int rows_in_block = (int)(blockDim.x >> 6) * RowIds<LPR>::RPW;
        const int k = (int)threadIdx.x;
        double bf = k < rows_in_block ? sf[k] : __builtin_huge_val();
        int64_t bi = k < rows_in_block ? si[k] : INT64_MAX;
        wave_argmin_ordered(bf, bi);
        if (k == 0) {
            part_f[id.block] = bf;
            part_i[id.block] = bi;
        }
    }
}

// ---- the one-workgroup steps behind a generation (sx_core.hip: argmin, best / termination; sx_runs_unfused.hip: one such
//      workgroup per run): kFinalWorkgroup threads reduce records by np.argmin's first-minimum rule
constexpr int kFinalWorkgroup = 256;

__device__ __forceinline__ void block_argmin(double &bf, int64_t &bi, double *sf, int64_t *si) {
    wave_argmin_all(bf, bi);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        sf[w] = bf;
        si[w] = bi;
    }
    __syncthreads();
    bf = sf[0];
    bi = si[0];
    for (int k = 1; k < kFinalWorkgroup / kWave; ++k) argmin_combine(bf, bi, sf[k], si[k]);
    __syncthreads();
}

// the termination ladder of the synchronous loops (_common.py:131-158) after generation `it`: dx = step of the best row,
// best = its value.  The one-thread / one-workgroup epilogues call this; the kernels that spell it out themselves say so
__device__ __forceinline__ int sync_status(double dx, double xtol, double best, double ftol, int64_t it, int64_t maxiter) {
    if (dx <= xtol && best <= ftol) return 0;
    if (best <= ftol) return 1;
    if (it >= maxiter) return -1;
    return SX_STATUS_NONE;
}

// best of the per-workgroup records, 8 records per thread and trip so their loads overlap
template <int kScan>
__device__ __forceinline__ void scan_records_n(const double *__restrict__ part_f, const int64_t *__restrict__ part_i,
                                               int64_t npart, double &bf, int64_t &bi) {
    for (int64_t k0 = threadIdx.x; k0 < npart; k0 += (int64_t)kFinalWorkgroup * kScan) {
        double f[kScan];
        int64_t i[kScan];
#pragma unroll
        for (int u = 0; u < kScan; ++u) {
            const int64_t k = k0 + (int64_t)u * kFinalWorkgroup;
            f[u] = k < npart ? part_f[k] : __builtin_huge_val();
            i[u] = k < npart ? part_i[k] : INT64_MAX;
        }
        // this trip's minimum in np.argmin's order (a tree), then the first record that holds it (k grows with u), then
        // one lexicographic step into the running pair: a chain of 8 compare-and-select steps otherwise
        double m = f[0];
#pragma unroll
        for (int u = 1; u < kScan; ++u) m = best_min(m, f[u]);  // (the minimum is the same in any order)
        int64_t first = i[0];
        double fm = f[0];  // (its own bits: the sign of a zero)
#pragma unroll
        for (int u = kScan - 1; u >= 0; --u)
            if (best_tie(f[u], m)) first = i[u], fm = f[u];
        argmin_combine(bf, bi, fm, first);
    }
}
// 8 records per thread and trip; all of config 5 on one GPU (131 072 rows = 16 384 records, 64 per thread) 32: two trips
// instead of eight dependent ones
__device__ __forceinline__ void scan_records(const double *__restrict__ part_f, const int64_t *__restrict__ part_i,
                                             int64_t npart, double &bf, int64_t &bi) {
    if (npart > (int64_t)kFinalWorkgroup * 16)
        scan_records_n<32>(part_f, part_i, npart, bf, bi);
    else
        scan_records_n<8>(part_f, part_i, npart, bf, bi);
}

// ---- DE donor rows (shared by the synchronous and the sequential kernels)
constexpr int kMaxDonors = 5;

__host__ __device__ inline int donors_of(int strategy) {
    return strategy == SX_DE_RAND1BIN ? 3 : strategy == SX_DE_RAND2BIN ? 5 : strategy == SX_DE_BEST1BIN ? 2 : 4;
}

// Philox donors: k distinct rows != i, uniform without replacement.  Word 1+t of the
// donor calls gives r_t = mulhi(w, P-1-t); r_t is then shifted past the
// sorted exclusion list {i, d_0..d_{t-1}} (oracle/streams.py PhiloxStream.de_generation).
__device__ __forceinline__ void philox_donors(int64_t P, int k, int64_t i, uint32_t grow, uint32_t gen, uint32_t k0,
                                              uint32_t k1, int n, int64_t (&d)[kMaxDonors], int &irand) {
    // word 0 -> forced crossover index, word 1+t -> donor t; the second call only for 4- and 5-donor strategies
    const U4 a = philox4x32_10(0u, grow, gen, kPurposeDeDonor, k0, k1);
    U4 b = {0u, 0u, 0u, 0u};
    if (k > 3) b = philox4x32_10(1u, grow, gen, kPurposeDeDonor, k0, k1);
    const uint32_t w[5] = {a.y, a.z, a.w, b.x, b.y};
    uint32_t excl[kMaxDonors + 1];  // P < 2^31 (checked on the host): 32-bit index arithmetic
    excl[0] = (uint32_t)i;
    const uint32_t Pm1 = (uint32_t)(P - 1);
#pragma unroll
    for (int t = 0; t < kMaxDonors; ++t) {
        if (t < k) {
            uint32_t v = __umulhi(w[t], Pm1 - (uint32_t)t);
#pragma unroll
            for (int s = 0; s <= t; ++s) v += (v >= excl[s]) ? 1u : 0u;
            d[t] = (int64_t)v;
            uint32_t carry = v;  // insert v into the sorted list excl[0..t]
#pragma unroll
            for (int s = 0; s <= t; ++s) {
                if (carry < excl[s]) {
                    const uint32_t tmp = excl[s];
                    excl[s] = carry;
                    carry = tmp;
                }
            }
            excl[t + 1] = carry;
        } else {
            d[t] = 0;
        }
    }
    irand = (int)__umulhi(a.x, (uint32_t)n);
}

// mutant of one element (de/_strategy.py:1-38, the reference's association order; no FMA): g = best row,
// d0..d4 = donor rows
__device__ __forceinline__ double de_mutant(int strategy, double g, double d0, double d1, double d2, double d3,
                                            double d4, double F) {
    if (strategy == SX_DE_BEST1BIN) return g + F * (d0 - d1);
    if (strategy == SX_DE_RAND1BIN) return d0 + F * (d1 - d2);
    if (strategy == SX_DE_BEST2BIN) return g + F * (((d0 + d1) - d2) - d3);
    return d0 + F * (((d1 + d2) - d3) - d4);
}

// new velocity of one element (cpso/_cpso.py:326, left to right): w*v + c1*r1*(p - x) + c2*r2*(g - x)
__device__ __forceinline__ double pso_velocity(double w, double v, double c1, double r1, double p, double x, double c2,
                                               double r2, double g) {
    return (w * v + (c1 * r1) * (p - x)) + (c2 * r2) * (g - x);
}

// Element e of row gi of the Philox-mode initial population of P rows (the Latin hypercube of _common.py:109-120, described at
// philox_lhs_kernel in sx_core.hip): shared by that kernel and the resident DE runs (sx_de_runs.hip), which draw a run's
// hypercube themselves -- one function, so the same bits.
__device__ __forceinline__ double philox_lhs_element(uint64_t gi, int e, int64_t P, int n, double lo, double hi, uint32_t k0,
                                                     uint32_t k1) {
    // the column's permutation keys
    const U4 ka = philox4x32_10((uint32_t)e, 0u, 0u, kPurposeInitPerm, k0, k1);
    const U4 kb = philox4x32_10((uint32_t)e, 1u, 0u, kPurposeInitPerm, k0, k1);
    const uint64_t m[3] = {(uint64_t)(ka.x | 1u), (uint64_t)(ka.y | 1u), (uint64_t)(ka.z | 1u)};
    const uint64_t ad[3] = {(uint64_t)kb.x, (uint64_t)kb.y, (uint64_t)kb.z};
    int b = 1;
    while (((uint64_t)1 << b) < (uint64_t)P) ++b;  // P >= 2: b = bit_length(P - 1)
    const uint64_t mask = ((uint64_t)1 << b) - 1u;
    const int sh = (b + 1) / 2;
    uint64_t x = gi;
    do {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            x = (x * m[k] + ad[k]) & mask;
            x ^= x >> sh;
        }
    } while (x >= (uint64_t)P);
    const double u = philox_u53(e, lanes_per_row(n), (uint32_t)gi, 0u, kPurposeInitJitter, k0, k1);
    const double step = 2.0 / (double)P;                      // np.linspace(-1, 1, P, endpoint=False): arange * step + start
    const double v = u / (double)P + ((double)x * step + -1.0);
    return v * (0.5 * (hi - lo)) + 0.5 * (hi + lo);
}

// run `body(std::integral_constant<int, LPR>)` for the LPR that lanes_per_row(n) prescribes
#define SX_DISPATCH_LPR(n, CALL)            \
    switch (lanes_per_row(n)) {             \
        case 16: { constexpr int LPR = 16; CALL; } break; \
        case 32: { constexpr int LPR = 32; CALL; } break; \
        default: { constexpr int LPR = 64; CALL; } break; \
    }

// run CALL with `constexpr int FUN` bound to the objective `fun_id` names (checked by the caller: 0 <= fun_id < SX_FUN_COUNT)
#define SX_DISPATCH_FUN(fun_id, CALL)                                                           \
    switch (fun_id) {                                                                           \
        case SX_FUN_ACKLEY: { constexpr int FUN = SX_FUN_ACKLEY; CALL; } break;                 \
        case SX_FUN_GRIEWANK: { constexpr int FUN = SX_FUN_GRIEWANK; CALL; } break;             \
        case SX_FUN_QUARTIC: { constexpr int FUN = SX_FUN_QUARTIC; CALL; } break;               \
        case SX_FUN_RASTRIGIN: { constexpr int FUN = SX_FUN_RASTRIGIN; CALL; } break;           \
        case SX_FUN_ROSENBROCK: { constexpr int FUN = SX_FUN_ROSENBROCK; CALL; } break;         \
        case SX_FUN_SPHERE: { constexpr int FUN = SX_FUN_SPHERE; CALL; } break;                 \
        default: { constexpr int FUN = SX_FUN_STYBLINSKI_TANG; CALL; } break;                   \
    }

}  // namespace sx
