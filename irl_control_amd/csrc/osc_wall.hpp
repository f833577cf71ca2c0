// COMPLIANT WALLS of a rollout (irlosc_set_walls): the wall of the reference's force_test scene as a penalty force on an end-effector
// body -- a half-space n.x >= off with stiffness k and damping c, the EE a sphere of radius r around the EE body's frame origin (the
// point the controller controls).  Unlike a push (osc_push.hpp) the force is computed on the device, per robot and per tick, from the
// EE position and velocity the walk has just produced, and remembered for one tick.  Two launches of one kernel per tick:
//
//   APPLY, behind the give-up pass, the waypoint cycler and the pushes' APPLY, in front of the plant: per device d with walls, in
//       ascending d,
//           x   = the EE xyz of this tick's walk (three entries at PlantArgs::ee0[d] of the exchange block)
//           v_c = sum_i J_d[c][i] qvel_i, c = 0..2, over the hinges above the EE body in ascending i: the jacp entries the walk parked
//                 behind the pose, qvel from the slot's qt as this tick's walk read it
//       and per wall w (table row nx ny nz off r k c 0) in ascending w
//           g = r - ((n0 x0 + n1 x1 + n2 x2) - off),   s = n0 v0 + n1 v1 + n2 v2,   f = k g - c s
//           F_w = (g > 0 && f > 0) ? f n : 0                 (a wall never pulls; a NaN anywhere: no contact, no force)
//       F_d = the sum of F_w in ascending w.  Float64 whatever the record type, every product, add and subtract rounded on its own, sums
//       left to right, the first term taken as it is: the host can repeat it (walls.py).  Then, unless F_d is all zero, for every
//       hinge i above the EE body   bias_i = fma(-J_d[2][i], F2, fma(-J_d[1][i], F1, fma(-J_d[0][i], F0, bias_i)))   in place on the
//       tick's exchange block (nothing between the walk and the plant writes J or the bias: DESIGN.md section 4.3), and F_d and the
//       counters go into the per-robot state, zeros included.
//   SENSE, between the pushes' SENSE and the action kernel, on every tick after the first: per device d with walls and a sensor,
//       wrench[b][d][c] = (T)((double)wrench[b][d][c] - F_d(t - 1)[c]), c = 0..2, F_d(t - 1) the stored force; the torque words are
//       untouched (the force acts at the frame origin, where the wrench is taken).
//
// One lane per robot, one block per walk wave (its 64 robots), like the push kernel.  A per-robot table is [walk wave][W 8][64] (every
// operand one coalesced 512-byte line), a shared one [W][8] (scalar loads); the state is SoA [ndev][stride].  The entry indices of J
// and the bias are compile-time constants of FeTopo<TOPO> per EE-candidate body; the runtime device finds its body by a uniform branch
// over the candidates.  No LDS.  Idle lanes of a ragged last wave neither load nor store.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/irlosc.h"
#include "osc_frontend_lane.hpp"

namespace irlosc {

struct WallState {            // the walls' per-robot state
    double* force;            // [3][ndev][stride]: what the last tick applied
    double* max_depth;        // [ndev][stride]: the largest g > 0 seen, or 0
    int32_t* contact_ticks;   // [ndev][stride]: ticks on which a wall of the device had g > 0
    int32_t* first_tick;      // [ndev][stride]: the first such tick, or -1
};
// One robot's fresh wall state (so: its column): what the fills of irlosc_set_walls leave, written by a reset of episodes
__device__ __forceinline__ void wall_fresh(WallState st, int ndev, int stride, size_t so) {
    const size_t plane = (size_t)ndev * stride;
    for (int d = 0; d < ndev; ++d) {
        const size_t o = (size_t)d * stride + so;
#pragma unroll
        for (int c = 0; c < 3; ++c) st.force[c * plane + o] = 0.0;
        st.max_depth[o] = 0.0; st.contact_ticks[o] = 0; st.first_tick[o] = -1;
    }
}

struct WallArgs {
    double* xside;            // apply: the tick's exchange block [walk wave][n_compact][64], bias entries in place
    const double* qt;         // apply: the slot's coordinates in the walk's layout [walk wave][2 NJ][64] (entry 2 i + 1 = qvel_i)
    void* wrench;             // sense: the feed's wrench of the tick [B][ndev][6], record type, xyz in place
    const double* table;      // per_robot: [walk wave][W][8][64], else [W][8]
    WallState st;
    int32_t B, ndev, W, per_robot, stride;
    int32_t apply;            // 1: apply mode, 0: sense mode (uniform over the launch)
    int32_t tick;             // apply: the walls' tick
    uint32_t devs;            // bit d: device d is part of this launch (apply: it has a wall; sense: and a sensor)
    int32_t dev[IRLOSC_MAX_WALLS];        // target device of wall w
    int32_t ee0[IRLOSC_MAX_DEV];          // exchange entry of each device's EE pose: names its EE body
};

template <class TOPO, typename T>
__global__ __launch_bounds__(64) void osc_wall_kernel(const WallArgs a) {
    using TI = FeTopo<TOPO>;
    constexpr int n_compact = TI::n_compact();
    constexpr int NJ = TOPO::NJ;
    const int lane = threadIdx.x;
    const int b = (int)blockIdx.x * 64 + lane;
    if (b >= a.B) return;                           // (no barrier below)
    const size_t plane = (size_t)a.ndev * a.stride;
    if (!a.apply) {
        for (int d = 0; d < a.ndev; ++d) {          // (uniform: a kernel argument)
            if (!((a.devs >> d) & 1u)) continue;
            const size_t so = (size_t)d * a.stride + b;
            T* w = (T*)a.wrench + ((size_t)b * a.ndev + d) * 6;
#pragma unroll
            for (int c = 0; c < 3; ++c) w[c] = (T)__dsub_rn((double)w[c], a.st.force[c * plane + so]);
        }
        return;
    }
    const double* __restrict__ tab = a.per_robot ? a.table + (size_t)blockIdx.x * a.W * 8 * 64 + lane : a.table;
    const int cs = a.per_robot ? 64 : 1;
    double* col = a.xside + (size_t)blockIdx.x * n_compact * 64 + lane;
    const double* __restrict__ gq = a.qt + (size_t)blockIdx.x * (2 * NJ * 64) + lane;
    for (int d = 0; d < a.ndev; ++d) {
        if (!((a.devs >> d) & 1u)) continue;
        const int e0d = a.ee0[d];
        const size_t so = (size_t)d * a.stride + b;
        static_for<0, TOPO::NB>([&](auto bc) {
            constexpr int body = decltype(bc)::value;
            if constexpr (TOPO::ee_cand[body] != 0) {
                constexpr int e0 = TI::ee_index(body);      // (indices through constexpr VARIABLES: evaluated at compile time)
                if (e0d == e0) {
                    constexpr int NA = TI::n_above(body);
                    const double x0 = col[(size_t)e0 * 64], x1 = col[(size_t)(e0 + 1) * 64], x2 = col[(size_t)(e0 + 2) * 64];
                    double J[NA > 0 ? NA : 1][3];
                    double v[3] = {0.0, 0.0, 0.0};
                    static_for<0, NJ>([&](auto ic) {
                        constexpr int i = decltype(ic)::value;
                        if constexpr (TI::moves(i, body)) {
                            constexpr int r = TI::anc_rank(i, body);
                            constexpr int ej = e0 + 7 + 6 * r;
                            const double qd = gq[(size_t)(2 * i + 1) * 64];
#pragma unroll
                            for (int c = 0; c < 3; ++c) {
                                J[r][c] = col[(size_t)(ej + c) * 64];
                                const double p = __dmul_rn(J[r][c], qd);
                                v[c] = r == 0 ? p : __dadd_rn(v[c], p);
                            }
                        }
                    });
                    double F[3] = {0.0, 0.0, 0.0};
                    double depth = 0.0;
                    bool first = true;
                    for (int w = 0; w < a.W; ++w) {      // (every condition uniform over the launch: kernel arguments)
                        if (a.dev[w] != d) continue;
                        const double* __restrict__ row = tab + (size_t)w * 8 * cs;
                        const double n0 = row[0], n1 = row[cs], n2 = row[2 * cs], off = row[3 * cs];
                        const double rad = row[4 * cs], k = row[5 * cs], cd = row[6 * cs];
                        const double nx = __dadd_rn(__dadd_rn(__dmul_rn(n0, x0), __dmul_rn(n1, x1)), __dmul_rn(n2, x2));
                        const double g = __dsub_rn(rad, __dsub_rn(nx, off));
                        const double s = __dadd_rn(__dadd_rn(__dmul_rn(n0, v[0]), __dmul_rn(n1, v[1])), __dmul_rn(n2, v[2]));
                        const double f = __dsub_rn(__dmul_rn(k, g), __dmul_rn(cd, s));
                        const bool on = g > 0.0 && f > 0.0;                  // NaN: no contact
                        const double Fw[3] = {on ? __dmul_rn(f, n0) : 0.0, on ? __dmul_rn(f, n1) : 0.0, on ? __dmul_rn(f, n2) : 0.0};
#pragma unroll
                        for (int c = 0; c < 3; ++c) F[c] = first ? Fw[c] : __dadd_rn(F[c], Fw[c]);
                        first = false;
                        if (g > depth) depth = g;
                    }
                    if (F[0] != 0.0 || F[1] != 0.0 || F[2] != 0.0) {
                        static_for<0, NJ>([&](auto ic) {
                            constexpr int i = decltype(ic)::value;
                            if constexpr (TI::moves(i, body)) {
                                constexpr int r = TI::anc_rank(i, body);
                                constexpr int eb = TI::bias_index(i);
                                double acc = col[(size_t)eb * 64];
#pragma unroll
                                for (int c = 0; c < 3; ++c) acc = fma(-J[r][c], F[c], acc);
                                col[(size_t)eb * 64] = acc;
                            }
                        });
                    }
#pragma unroll
                    for (int c = 0; c < 3; ++c) a.st.force[c * plane + so] = F[c];
                    if (depth > 0.0) {
                        if (depth > a.st.max_depth[so]) a.st.max_depth[so] = depth;
                        a.st.contact_ticks[so] += 1;
                        if (a.st.first_tick[so] < 0) a.st.first_tick[so] = a.tick;
                    }
                }
            }
        });
    }
}

}  // namespace irlosc
