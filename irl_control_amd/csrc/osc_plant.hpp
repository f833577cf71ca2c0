// The contact-free PLANT of the fused path (irlosc_rollout_from_q): behind a fused step from joint coordinates, every robot's
//     qacc = M^-1 (u - bias - damping qvel);   qvel += dt qacc;   qpos += dt qvel          (semi-implicit Euler)
// written back into the slot's coordinates, so that the next tick's walk starts from them without the host in between.  Not a simulator:
// no contacts; joint limits, the gripper's equality rows and a driven gripper only as the penalty rows of irlosc_set_joints, which reach
// this kernel through the bias (osc_joint.hpp) -- the plant examples/closed_loop_headless.py integrates in NumPy.
//
// One lane per robot, one block per walk wave (its 64 robots), float64 arithmetic whatever the record type.  Everything it needs is in
// HBM after the step: the walk left the tree's non-zeros of M, the bias forces and the EE poses in the step's exchange block
// ([walk wave][entry][64 robots]: every operand one coalesced 512-byte load, compile-time entry indices of FeTopo<TOPO>), the OSC step
// (or the give-up pass behind it) left u[B][n] row-major in the record type: a wave's 64 x NJ tile is transposed through LDS.
//
//   M = L^T L from the leaves up (hinges NJ-1 .. 0, no fill-in: the recursion of osc_lane.hpp without M dq, Y and the pins): row j of M is read when
//       hinge j is eliminated, L[j][i] = (m_ji - Delta[j][i]) / L[j][j], Delta[a][b] += L[j][a] L[j][b] for the hinges a, b above j;
//   L^T y = rhs rides along (rhs_i -= L[j][i] y_j), rhs_j = (ctrl_mask bit j ? u_j : 0) - bias_j - damping qvel_j;
//   L qacc = y from the root down needs the rows of L again in ASCENDING order.  155 off-diagonal entries + 25 pivots are 360
//       registers; they go back where the row of M came from instead -- the exchange block is scratch once the step's give-up pass has
//       run, each lane owns its column of it, and the block is rewritten by the next walk -- which keeps the kernel at two waves per
//       SIMD (tools/kernel_regs.py) at the price of 1.4 KB per robot written and read once more.
// A robot whose u is not finite, whose pivot is not positive or whose qacc is not finite is FROZEN: its coordinates are stored back
// unchanged and IRLOSC_FLAG_NONFINITE (resp. IRLOSC_FLAG_M_NOT_PD) goes into flags_any; per-lane selects, no divergent exit, so its
// wave mates are unaffected.  Outputs: qt in place AND the slot's row-major qpos / qvel (both copies stay in step), optionally the EE
// poses the walk computed -- those at the START of this tick -- into a trace sample, and flags_any |= flags of the tick.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/irlosc.h"
#include "osc_frontend_lane.hpp"

namespace irlosc {

struct PlantArgs {
    double* xside;            // the step's exchange block [walk wave][n_compact][64]; the M entries are overwritten (factor L)
    const void* u;            // [B][NJ] torques of the step, record type
    const uint32_t* flags;    // [B] flags of the step
    double* qt;               // [walk wave][2 NJ][64]: in place
    double* qpos;             // [B][NJ] row-major: in place
    double* qvel;
    double* trace;            // [B][ndev][7] EE poses of this tick, or nullptr
    uint32_t* flags_any;      // [B]: |= flags of the tick | what the plant itself found
    double dt, damping;
    uint32_t ctrl_mask;
    int32_t B, ndev;
    int32_t ee0[IRLOSC_MAX_DEV];      // exchange entry of each device's EE pose (x y z qw qx qy qz follow each other)
};

template <class TOPO, typename TIN>
__global__ __launch_bounds__(64, 2) void osc_plant_lane_kernel(const PlantArgs a) {
    using TI = FeTopo<TOPO>;
    constexpr int NJ = TOPO::NJ;
    constexpr int NE = TI::n_pairs() + NJ;          // M's entries of the block: the pairs, then the diagonal
    constexpr int n_compact = TI::n_compact();
    constexpr int PFD = 1;                          // rows requested ahead of the one being eliminated
    __shared__ double s_t[64 * NJ];                 // the wave's u tile, then its qvel and qpos tiles on the way out
    const int lane = threadIdx.x;
    const int b0 = (int)blockIdx.x * 64;
    const int nvalid = min(64, a.B - b0);           // robots of this wave (a ragged last wave: its idle lanes store nothing)
    const bool valid = lane < nvalid;
    double* __restrict__ col = a.xside + (size_t)blockIdx.x * n_compact * 64 + lane;
    double* __restrict__ qcol = a.qt + (size_t)blockIdx.x * (2 * NJ * 64) + lane;

    // u: the wave's tile is nvalid * NJ consecutive values -- coalesced loads, then each lane picks its row out of LDS
    {
        const TIN* __restrict__ ug = (const TIN*)a.u + (size_t)b0 * NJ;
#pragma unroll
        for (int t = 0; t < NJ; ++t) {
            const int idx = t * 64 + lane;
            s_t[idx] = idx < nvalid * NJ ? (double)ug[idx] : 0.0;
        }
    }
    __syncthreads();
    double rhs[NJ];
    bool bad_u = false;
    // (indices through constexpr VARIABLES throughout: a constexpr function call in a runtime expression is evaluated at run time)
    constexpr int bias0 = TI::bias_index(0);
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const double uj = s_t[lane * NJ + j];
        bad_u = bad_u | !(fabs(uj) <= 1.7976931348623157e308);        // NaN or infinite
        const double ctrl = ((a.ctrl_mask >> j) & 1u) ? uj : 0.0;
        rhs[j] = (ctrl - col[(size_t)(bias0 + j) * 64]) - a.damping * qcol[(2 * j + 1) * 64];
    }
    // the EE poses of this tick (a traced tick only: uniform over the launch)
    if (a.trace && valid) {
        double* tr = a.trace + (size_t)(b0 + lane) * a.ndev * 7;
        for (int d = 0; d < a.ndev; ++d)
#pragma unroll
            for (int c = 0; c < 7; ++c) tr[d * 7 + c] = col[(size_t)(a.ee0[d] + c) * 64];
    }
    __builtin_amdgcn_sched_barrier(0);

    // ---- M = L^T L and L^T y = rhs, hinges NJ - 1 .. 0 ------------------------------------------------------------------------------
    double Mv[NE], Dl[NE], lrow[NJ];
    const double* src = col;
    auto fetch = [&](auto jc) {
        constexpr int j = decltype(jc)::value;
        static_for<0, j + 1>([&](auto ic) {
            constexpr int i = decltype(ic)::value;
            if constexpr (TI::above(i, j)) {
                constexpr int e = TI::m_entry(i, j);
                Mv[e] = src[(size_t)e * 64];
            }
        });
    };
    static_for_down<NJ - PFD < 0 ? 0 : NJ - PFD, NJ>([&](auto jc) { fetch(jc); });
    bool npd = false;
    static_for_down<0, NJ>([&](auto jc) {
        constexpr int j = decltype(jc)::value;
        if constexpr (j - PFD >= 0) fetch(std::integral_constant<int, (j - PFD >= 0 ? j - PFD : 0)>{});
        __builtin_amdgcn_sched_barrier(0);
        constexpr int ed = TI::diag_index(j);
        constexpr bool below = TI::has_below(j);
        double d = Mv[ed];
        if constexpr (below) d -= Dl[ed];
        npd = npd | !(d > 0.0);                                // also catches NaN
        d = fmax(d, 1e-300);
        const double rs = rsq_refined(d);
        const double yj = rhs[j] * rs;
        rhs[j] = yj;                                           // y_j from here on
        col[(size_t)ed * 64] = rs;                             // 1 / L[j][j] in place of M[j][j]
        static_for<0, j>([&](auto ic) {
            constexpr int i = decltype(ic)::value;
            if constexpr (TI::above(i, j)) {
                constexpr int e = TI::pair_index(i, j);
                const double m = below ? Mv[e] - Dl[e] : Mv[e];
                const double l = m * rs;                       // L[j][i]
                lrow[i] = l;
                col[(size_t)e * 64] = l;                       // in place of M[j][i]
                rhs[i] = fma(-l, yj, rhs[i]);                  // L^T y = rhs: what hinge j takes out of its ancestors' rows
            }
        });
        static_for<0, j>([&](auto ac) {
            constexpr int ai = decltype(ac)::value;
            if constexpr (TI::above(ai, j)) {
                constexpr int alast = TI::subtree_last(ai);
                static_for<0, ai + 1>([&](auto bc) {
                    constexpr int bi = decltype(bc)::value;
                    if constexpr (TI::above(bi, j)) {
                        constexpr int e = TI::m_entry(bi, ai);
                        // the first hinge (in this order) under both: the last index of the deeper one's subtree
                        if constexpr (alast == j) Dl[e] = lrow[ai] * lrow[bi];
                        else Dl[e] = fma(lrow[ai], lrow[bi], Dl[e]);
                    }
                });
            }
        });
    });
    __builtin_amdgcn_sched_barrier(0);

    // ---- L qacc = y, hinges 0 .. NJ - 1: row j of L comes back from the block (this lane's own stores) --------------------------------
    // (the address laundered: a compiler that sees the stores above forwards all 180 values to these loads -- in registers)
    asm volatile("" : "+v"(src) : : "memory");
    static_for<0, (PFD < NJ ? PFD : NJ)>([&](auto jc) { fetch(jc); });
    bool bad_a = false;
    static_for<0, NJ>([&](auto jc) {
        constexpr int j = decltype(jc)::value;
        if constexpr (j + PFD < NJ) fetch(std::integral_constant<int, (j + PFD < NJ ? j + PFD : 0)>{});
        __builtin_amdgcn_sched_barrier(0);
        double x = rhs[j];
        static_for<0, j>([&](auto ic) {
            constexpr int i = decltype(ic)::value;
            if constexpr (TI::above(i, j)) {
                constexpr int e = TI::pair_index(i, j);
                x = fma(-Mv[e], rhs[i], x);
            }
        });
        constexpr int ed = TI::diag_index(j);
        x *= Mv[ed];
        rhs[j] = x;                                            // qacc_j
        bad_a = bad_a | !(fabs(x) <= 1.7976931348623157e308);
    });

    // ---- semi-implicit Euler; a frozen robot keeps its coordinates bit for bit --------------------------------------------------------
    const bool frozen = bad_u | npd | bad_a;
    const uint32_t mine = ((bad_u | bad_a) ? IRLOSC_FLAG_NONFINITE : 0u) | (npd ? IRLOSC_FLAG_M_NOT_PD : 0u);
    // (the coordinates are read again here, behind the laundering above, instead of living in 100 registers across the recursion)
    double q[NJ], qd[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        q[j] = qcol[(2 * j) * 64];
        qd[j] = qcol[(2 * j + 1) * 64];
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const double v = fma(a.dt, rhs[j], qd[j]);
        const double p = fma(a.dt, v, q[j]);
        qd[j] = frozen ? qd[j] : v;
        q[j] = frozen ? q[j] : p;
    }
    if (valid) {
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            qcol[(2 * j) * 64] = q[j];
            qcol[(2 * j + 1) * 64] = qd[j];
        }
        a.flags_any[b0 + lane] |= a.flags[b0 + lane] | mine;
    }
    // row-major copies: each tile through LDS, stored as nvalid * NJ consecutive doubles
    double* __restrict__ outs[2] = {a.qvel + (size_t)b0 * NJ, a.qpos + (size_t)b0 * NJ};
#pragma unroll
    for (int w = 0; w < 2; ++w) {
        __syncthreads();
#pragma unroll
        for (int j = 0; j < NJ; ++j) s_t[lane * NJ + j] = w == 0 ? qd[j] : q[j];
        __syncthreads();
#pragma unroll
        for (int t = 0; t < NJ; ++t) {
            const int idx = t * 64 + lane;
            if (idx < nvalid * NJ) outs[w][idx] = s_t[idx];
        }
    }
}

}  // namespace irlosc
