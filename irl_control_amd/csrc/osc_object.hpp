// The ACTION OBJECTS of a rollout (irlosc_set_objects): kinematic bodies that a gripper carries -- per tick and robot, a held object
// rides rigidly on the EE that holds it, a free one is taken by a hand that closes near it, one that is let go stays where it is, and a
// plug that is free inside its socket's tolerances is recorded as mated.  NO contact model: this kernel moves poses and nothing else --
// a held object's weight on the plant and in the F/T feed is osc_object_load.hpp's, on a slot with loads -- and nothing collides, falls or
// slips.  It runs behind the walk (and the feed's SENSE launches) and in front of the
// action kernel: a WP entered on tick t (osc_action.hpp, refs) reads the objects of tick t.
//
// One lane per robot, one block per walk wave (its 64 robots), like the action kernel.  The EE pose of a gripper's device is seven
// coalesced 512-byte loads of the tick's exchange block [walk wave][entry][64]; the knuckle coordinate is entry 2 j of the slot's
// coordinates in the walk's layout [walk wave][2 n][64]: what the tick's walk read.  Per-robot state is SoA [row][stride]; a lane only
// touches its own column, so what it wrote in an earlier phase it reads back from there.  The arithmetic is float64 whatever the record
// type, only + - x, comparisons and quat2mat_rn's one division, every product and sum rounded on its own and in the order written here:
// the host repeats it bit for bit (irl_control_amd/objects.py::object_step).  No sqrt, no trigonometry, no normalisation; distances are
// compared squared.
//
// Gripper g (device dev[g], knuckle hinge joint[g], q its coordinate at the start of the tick):
//   closed = sign q >= sign q_close;  open = sign q <= sign q_open;  a NaN is neither.
// Per robot on tick t, with T_ee(g) = (p_ee, q_ee) the EE pose of dev[g] and R = quat2mat_rn:
//   0. a word of a gripper's EE pose that is not finite: the robot's objects, grippers and mates stay as they are on this tick
//   1. held objects, ascending o (holder h):  h open -> holder = -1, release_tick = t, the pose stays;
//        else xyz = p_ee + R(q_ee) rel_xyz, quat = q_ee (x) rel_quat
//   2. free objects not released on this tick, ascending o, grippers ascending g:  g closed, was_closed[g] == 0 (the rising edge: a hand
//        that travels closed picks nothing up), g holds nothing, |p_ee + R(q_ee) grip_xyz - p_obj|^2 <= radius^2
//        -> holder = g, rel_xyz = R(q_ee)^T (p_obj - p_ee), rel_quat = conj(q_ee) (x) q_obj, grasp_tick = t
//   3. was_closed[g] = closed(g)
//   4. mates, ascending m, with mated_tick < 0 and the plug free:  target xyz = p_sock + R(q_sock) seat_xyz, quat = q_sock (x) seat_quat;
//        |p_plug - target|^2 <= tol_xyz^2 and |q_plug . q_target| >= min_abs_dot -> mated_tick = t
//
// init = 1 (irlosc_set_objects): every robot's state fresh on variant 0 of `pose0` (object_fresh); no block or coordinate is read.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/irlosc.h"
#include "osc_common.hpp"

namespace irlosc {

// THE LAYOUT of the objects' per-robot state, for the kernels that read it (osc_action.hpp, osc_log.hpp, osc_episode.hpp) and the host:
// doubles in rows of `stride` words, pose word c of object o in row o 7 + c, rel behind the poses; ints likewise, by field
constexpr int OBJ_POSE_ROWS = IRLOSC_MAX_OBJECTS * 7;
constexpr int OBJ_D_ROWS = 2 * OBJ_POSE_ROWS;
constexpr int OBJ_I_ROWS = 3 * IRLOSC_MAX_OBJECTS + IRLOSC_MAX_GRIPPERS + IRLOSC_MAX_MATES;

struct ObjectState {          // the objects' per-robot state (the layout above)
    double* pose; double* rel;                                      // [MAX_OBJECTS 7][stride] each
    int32_t* holder; int32_t* grasp_tick; int32_t* release_tick;    // [MAX_OBJECTS][stride] each
    int32_t* was_closed; int32_t* mated_tick;                       // [MAX_GRIPPERS][stride], [MAX_MATES][stride]
};
// One robot's fresh object state (b: its column of rows S words apart) on the start poses at p0, the robot's column of a variant's
// [nobj 7][64] lines: what the init launch of irlosc_set_objects leaves on variant 0, and a reset of episodes on the variant it picks
__device__ __forceinline__ void object_fresh(ObjectState st, const double* p0, int nobj, int ng, int nm, size_t S, size_t b) {
    for (int o = 0; o < nobj; ++o) {
#pragma unroll
        for (int c = 0; c < 7; ++c) { st.pose[(size_t)(o * 7 + c) * S + b] = p0[(size_t)(o * 7 + c) * 64]; st.rel[(size_t)(o * 7 + c) * S + b] = 0.0; }
        st.holder[o * S + b] = -1; st.grasp_tick[o * S + b] = -1; st.release_tick[o * S + b] = -1;
    }
    for (int g = 0; g < ng; ++g) st.was_closed[g * S + b] = 0;
    for (int m = 0; m < nm; ++m) st.mated_tick[m * S + b] = -1;
}

struct ObjectArgs {
    const double* xside;      // the tick's exchange block [walk wave][n_entries][64] (init: not read)
    const double* qt;         // the slot's coordinates in the walk's layout [walk wave][2 n][64] (init: not read)
    const double* pose0;      // init: [walk wave][nobj 7][64], variant 0 of the start poses; else not read
    ObjectState st;
    double sign[IRLOSC_MAX_GRIPPERS], q_close[IRLOSC_MAX_GRIPPERS], q_open[IRLOSC_MAX_GRIPPERS], grip_xyz[IRLOSC_MAX_GRIPPERS][3];
    double radius[IRLOSC_MAX_OBJECTS];
    double seat_xyz[IRLOSC_MAX_MATES][3], seat_quat[IRLOSC_MAX_MATES][4], tol_xyz[IRLOSC_MAX_MATES], min_abs_dot[IRLOSC_MAX_MATES];
    int32_t ee[IRLOSC_MAX_GRIPPERS][7];      // exchange entries of the gripper's device: x y z qw qx qy qz
    int32_t joint[IRLOSC_MAX_GRIPPERS], plug[IRLOSC_MAX_MATES], socket[IRLOSC_MAX_MATES];
    int32_t B, n, stride, nobj, ng, nm, n_entries, tick, init;
};

__device__ __forceinline__ double obj_dist2(const double a[3], const double b[3]) {
    const double dx = __dsub_rn(a[0], b[0]), dy = __dsub_rn(a[1], b[1]), dz = __dsub_rn(a[2], b[2]);
    return __dadd_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)), __dmul_rn(dz, dz));
}

template <int NG>      // the grippers a lane keeps in registers: IRLOSC_MAX_GRIPPERS (a template so that only tu_object.hip holds the kernel)
__global__ __launch_bounds__(64) void osc_object_kernel(const ObjectArgs a) {
    const int lane = threadIdx.x;
    const int b = (int)blockIdx.x * 64 + lane;
    if (b >= a.B) return;                           // (no barrier below; idle lanes of a ragged last wave neither load nor store)
    const size_t S = (size_t)a.stride;
    if (a.init) {
        object_fresh(a.st, a.pose0 + (size_t)blockIdx.x * a.nobj * 7 * 64 + lane, a.nobj, a.ng, a.nm, S, (size_t)b);
        return;
    }
    double* __restrict__ pose = a.st.pose + b;      // this robot's column: row r at [r S]
    double* __restrict__ rel = a.st.rel + b;
    int32_t* __restrict__ holder = a.st.holder + b;
    const double* __restrict__ xs = a.xside + (size_t)blockIdx.x * a.n_entries * 64 + lane;
    const double* __restrict__ gq = a.qt + (size_t)blockIdx.x * (2 * a.n * 64) + lane;
    // ---- the grippers of the tick: EE pose, R(q_ee), closed / open (compile-time g: registers) ----
    double pe[NG][3], qe[NG][4], R[NG][3][3];
    bool closed[NG], open[NG], holds[NG];
    bool bad = false;
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        closed[g] = open[g] = holds[g] = false;
        if (g < a.ng) {
#pragma unroll
            for (int c = 0; c < 7; ++c) {
                const double v = xs[(size_t)a.ee[g][c] * 64];
                if (c < 3) pe[g][c] = v; else qe[g][c - 3] = v;
                bad = bad || !t_finite(v);
            }
            quat2mat_rn(qe[g], R[g]);
            const double sq = __dmul_rn(a.sign[g], gq[(size_t)(2 * a.joint[g]) * 64]);
            closed[g] = sq >= __dmul_rn(a.sign[g], a.q_close[g]);      // NaN: neither
            open[g] = sq <= __dmul_rn(a.sign[g], a.q_open[g]);
        }
    }
    if (bad) return;                                // 0.
    // ---- 1. held objects ----
    uint32_t released = 0;                          // bit o: let go on this tick
    for (int o = 0; o < a.nobj; ++o) {
        const int h = holder[o * S];
        if (h < 0) continue;
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            if (h != g) continue;
            if (open[g]) {
                holder[o * S] = -1;
                a.st.release_tick[o * S + b] = a.tick;
                released |= 1u << o;
            } else {
                double rx[3], rq[4], v[3], q[4];
#pragma unroll
                for (int c = 0; c < 3; ++c) rx[c] = rel[(size_t)(o * 7 + c) * S];
#pragma unroll
                for (int c = 0; c < 4; ++c) rq[c] = rel[(size_t)(o * 7 + 3 + c) * S];
                mat_vec_rn(R[g], rx, v);
                quat_mul_rn(qe[g], rq, q);
#pragma unroll
                for (int c = 0; c < 3; ++c) pose[(size_t)(o * 7 + c) * S] = __dadd_rn(pe[g][c], v[c]);
#pragma unroll
                for (int c = 0; c < 4; ++c) pose[(size_t)(o * 7 + 3 + c) * S] = q[c];
                holds[g] = true;
            }
        }
    }
    // ---- 2. free objects: a hand that closes on this tick near one takes it ----
    for (int o = 0; o < a.nobj; ++o) {
        if (holder[o * S] >= 0 || ((released >> o) & 1u)) continue;
        double po[3], qo[4];
#pragma unroll
        for (int c = 0; c < 3; ++c) po[c] = pose[(size_t)(o * 7 + c) * S];
        const double r2 = __dmul_rn(a.radius[o], a.radius[o]);
        bool taken = false;
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            if (g >= a.ng || taken || !closed[g] || holds[g] || a.st.was_closed[g * S + b] != 0) continue;
            double gv[3], gp[3];
            mat_vec_rn(R[g], a.grip_xyz[g], gv);
#pragma unroll
            for (int c = 0; c < 3; ++c) gp[c] = __dadd_rn(pe[g][c], gv[c]);
            if (!(obj_dist2(gp, po) <= r2)) continue;      // NaN: no grasp
            double d[3], rx[3], rq[4];
#pragma unroll
            for (int c = 0; c < 3; ++c) d[c] = __dsub_rn(po[c], pe[g][c]);
            mat_t_vec_rn(R[g], d, rx);
#pragma unroll
            for (int c = 0; c < 4; ++c) qo[c] = pose[(size_t)(o * 7 + 3 + c) * S];
            const double qc[4] = {qe[g][0], -qe[g][1], -qe[g][2], -qe[g][3]};
            quat_mul_rn(qc, qo, rq);
#pragma unroll
            for (int c = 0; c < 3; ++c) rel[(size_t)(o * 7 + c) * S] = rx[c];
#pragma unroll
            for (int c = 0; c < 4; ++c) rel[(size_t)(o * 7 + 3 + c) * S] = rq[c];
            holder[o * S] = g;
            a.st.grasp_tick[o * S + b] = a.tick;
            holds[g] = true;
            taken = true;
        }
    }
    // ---- 3. the edge detector ----
#pragma unroll
    for (int g = 0; g < NG; ++g)
        if (g < a.ng) a.st.was_closed[g * S + b] = closed[g] ? 1 : 0;
    // ---- 4. mates ----
    for (int m = 0; m < a.nm; ++m) {
        if (a.st.mated_tick[m * S + b] >= 0 || holder[a.plug[m] * S] >= 0) continue;
        double pp[3], qp[4], ps[3], qs[4], Rs[3][3], sv[3], tp[3], tq[4];
#pragma unroll
        for (int c = 0; c < 3; ++c) { pp[c] = pose[(size_t)(a.plug[m] * 7 + c) * S]; ps[c] = pose[(size_t)(a.socket[m] * 7 + c) * S]; }
#pragma unroll
        for (int c = 0; c < 4; ++c) { qp[c] = pose[(size_t)(a.plug[m] * 7 + 3 + c) * S]; qs[c] = pose[(size_t)(a.socket[m] * 7 + 3 + c) * S]; }
        quat2mat_rn(qs, Rs);
        mat_vec_rn(Rs, a.seat_xyz[m], sv);
#pragma unroll
        for (int c = 0; c < 3; ++c) tp[c] = __dadd_rn(ps[c], sv[c]);
        quat_mul_rn(qs, a.seat_quat[m], tq);
        const double dot = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(qp[0], tq[0]), __dmul_rn(qp[1], tq[1])), __dmul_rn(qp[2], tq[2])), __dmul_rn(qp[3], tq[3]));
        if (obj_dist2(pp, tp) <= __dmul_rn(a.tol_xyz[m], a.tol_xyz[m]) && fabs(dot) >= a.min_abs_dot[m]) a.st.mated_tick[m * S + b] = a.tick;
    }
}

}  // namespace irlosc
