// The ACTION LIST of a rollout (irlosc_set_action_list): per tick and robot the WP / GRIP state machine of the insertion demo's fleet
// form (action_sequence.py::FleetActionSequenceRunner.tick + after_step) -- judge the active arm's task error on this tick's EE pose,
// advance, write the targets of an action that is entered, and set the error-adaptive velocity limit of the active arm in the slot's
// own gain copy -- so that the OSC step of the SAME tick aims at them without the host in between.  It runs between the walk (and the
// sensor feed's wrench) and the first OSC kernel of the tick; after_step, which needs the EE pose of the state the plant produced, is
// the start of the following tick: only the next walk has that pose.
//
// One lane per robot, one block per walk wave (its 64 robots), like the waypoint cycler.  The EE pose of the active and the passive
// device is seven coalesced 512-byte loads each of the tick's exchange block; the target record tgt[B][ndev][7] goes through the
// wave's target tile (osc_common.hpp: its contract), stored by a wave in which a lane entered a WP.  Per-robot state is SoA
// [field][stride]; a per-robot pose table is [walk wave][A][7][64], a shared one [A][7].  The error is float64 (task_error6<double>,
// the target words converted to double), its norm and the limit with every product and sum rounded on its own: the host can repeat them.
//
// Per robot on tick t of the list (A actions; a = action).  A robot's list starts on the FIRST TICK THAT RUNS IT (entered < 0: nothing
// entered yet) -- tick 0 for every robot of a rollout over the whole list, a later one for a robot that earlier, narrower rollouts left
// out: on that tick it is not judged, start_xyz is taken and action 0 is entered.  finished_tick counts the slot's ticks all the same.
//   1. not its first tick and a < A:  err = |calc_error(ee[active], tgt[active] as stored)|_2;  WP: err <= max_error[a] -> a += 1 (a NaN never advances);
//                        GRIP: grip_left -= 1, <= 0 -> a += 1;  a == A: finished_tick = t
//   2. its first tick:   start_xyz = EE xyz of the active device
//   3. a < A and entered != a:  entered = a, gripper_force = gripper_force[a];  WP: passive target = its EE xyz + (its EE quaternion |
//                        passive_quat), active target = pose a (xyz = start_xyz where xyz_from_start[a]), err = +inf;
//                        GRIP: grip_left = grip_ticks[a], targets stay
//   4. a < A and WP:     max_vel0 = max(min_speed[a], min(max_speed[a], kp[a] * err)) -> word 9 of the active device's gain record
// A robot that has finished holds its last targets and gains.
// REFS (irlosc_set_action_refs, on a slot with action objects: osc_object.hpp, whose kernel has run on this tick already).  A WP with
// xyz_obj[a] >= 0: the xyz words of pose a are an OFFSET, target xyz = the object's xyz + offset, one add per word (the reference's
// obj_pos + offset); xyz_from_start wins.  With quat_obj[a] >= 0 the quaternion words are the grip rotation, target quat = q_obj (x)
// q_grip (quat_mul_rn: no normalisation, no sign change) -- the reference reaches the same rotation through mat2euler -> set_abg, equal
// up to the quaternion's sign, which calc_error does not see.  Read at ENTRY only: a held object does not drag a target along.
//
// MOTION (irlosc_set_action_motion; the MOTION = true instantiation, launched only for a slot that has one -- the MOTION = false
// instantiation is the kernel above and nothing else).  Per action steps[a] (0: the WP jumps; N >= 1: INTERP, the target travels to the
// goal over N ticks) and noise_mean[a], noise_std[a]; per robot step, draws, origin[7], goal[7], SoA like the rest.
//   3'. entry of a WP:   the goal is composed as in 3. and KEPT IN FLOAT64; an action with noise (noise_std[a] > 0 or noise_mean[a] != 0):
//                        goal_c += noise_mean[a] + noise_std[a] * z_c for c in x, y, z, each product and sum rounded on its own, (z_0, z_1,
//                        z_2) = normal3(seed, robot's index in the slot, draws, a) (osc_rng.hpp), then draws += 1;  goal is stored,
//                        origin = the active device's EE pose of this tick, step = 0.  (A GRIP's entry writes none of them.)
//       steps[a] == 0:   target = goal in the record type, on the entry tick only
//       steps[a] = N:    on the entry tick and every later tick in this action with step < N:  step += 1, w = step / N;
//                        step < N:  xyz_c = origin_c + w * (goal_c - origin_c);  quaternion: both ends divided by their norms, the goal's
//                        sign flipped where their dot product is negative, the blend qa_c + w * (qb_c - qa_c) divided by its norm;
//                        step == N: the seven goal words as composed (no flip, no renormalisation: steps = 1 without noise is a WP)
//   1'. an INTERP action advances only when step == N and err <= max_error[a]; err is the error against the target as stored -- the
//       moving one -- and feeds the limit of 4. unchanged.
// A reset of episodes leaves entered = -1, which re-enters action 0 and with it rewrites goal, origin and step; draws is NOT reset, so
// that every episode of a robot draws fresh noise.
//
// init = 1 (irlosc_set_action_list): every robot's state fresh (list_fresh); neither the exchange block nor the targets are read.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/irlosc.h"
#include "osc_common.hpp"
#include "osc_rng.hpp"

namespace irlosc {

struct ListState {            // the list's per-robot state: [stride] each, start_xyz [3][stride]
    int32_t* action; int32_t* entered; int32_t* grip_left; int32_t* finished_tick;
    double* err; double* max_vel0; double* gripper_force; double* start_xyz;
};
// One robot's fresh list state (so: its column): what the init launch of irlosc_set_action_list leaves, and a reset of episodes
__device__ __forceinline__ void list_fresh(ListState st, int stride, size_t so) {
    st.action[so] = 0; st.entered[so] = -1; st.grip_left[so] = 0; st.finished_tick[so] = -1;
    st.err[so] = __builtin_huge_val(); st.max_vel0[so] = 0.0; st.gripper_force[so] = 0.0;
#pragma unroll
    for (int c = 0; c < 3; ++c) st.start_xyz[(size_t)c * stride + so] = 0.0;
}
// The motion's per-robot state: step and draws [stride], origin and goal [7][stride].  No fresh function: a reset leaves it alone (above)
struct MotionState { int32_t* m_step; uint32_t* m_draws; double* m_origin; double* m_goal; };

struct ActionArgs {
    const double* xside;      // the tick's exchange block [walk wave][n_entries][64] (init: not read)
    void* tgt;                // [B][ndev][7] targets of the slot, record type
    void* gains;              // [B][ndev][IRLOSC_GAIN_WORDS] the slot's gain copy, record type: word 9 of the active device in place
    ListState st;
    const double* table;      // per_robot: [walk wave][A][7][64], else [A][7]
    const double* obj_pose;   // REFS in force: the action objects' poses of this tick [IRLOSC_MAX_OBJECTS 7][stride] (osc_object.hpp); else nullptr
    double kp[IRLOSC_MAX_ACTIONS], max_error[IRLOSC_MAX_ACTIONS], min_speed[IRLOSC_MAX_ACTIONS], max_speed[IRLOSC_MAX_ACTIONS];
    double force[IRLOSC_MAX_ACTIONS];
    double passive_quat[4];
    int32_t grip_ticks[IRLOSC_MAX_ACTIONS];
    uint8_t kind[IRLOSC_MAX_ACTIONS], xyz_from_start[IRLOSC_MAX_ACTIONS];
    int8_t xyz_obj[IRLOSC_MAX_ACTIONS], quat_obj[IRLOSC_MAX_ACTIONS];      // refs: the object a WP's xyz / quaternion aims at, or -1
    int32_t ee_act[7], ee_pas[7];       // exchange entries of the active / passive device's x y z qw qx qy qz
    int32_t B, ndev, stride, A, per_robot, n_entries, tick, init;
    int32_t active, passive, hold;      // device indices (passive -1: none); hold: the passive arm keeps its EE orientation
};

// The arguments of the MOTION = true instantiation: the list's, and the motion in force (irlosc_set_action_motion)
struct ActionMotionArgs : ActionArgs {
    MotionState mo;
    double noise_mean[IRLOSC_MAX_ACTIONS], noise_std[IRLOSC_MAX_ACTIONS];
    int32_t steps[IRLOSC_MAX_ACTIONS];
    uint64_t seed;
};
static_assert(sizeof(ActionMotionArgs) <= 4096, "kernel arguments travel in a 4 KB segment");
template <bool MOTION> struct action_args_of { typedef ActionArgs type; };
template <> struct action_args_of<true> { typedef ActionMotionArgs type; };

// qa + w (qb - qa) between the normalised ends on the short arc, normalised (nlerp); every operation rounded on its own
__device__ __forceinline__ void quat_nlerp_rn(const double* o, const double* g, double w, double r[4]) {
    const double no = __dsqrt_rn(__dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(o[0], o[0]), __dmul_rn(o[1], o[1])), __dmul_rn(o[2], o[2])), __dmul_rn(o[3], o[3])));
    const double ng = __dsqrt_rn(__dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(g[0], g[0]), __dmul_rn(g[1], g[1])), __dmul_rn(g[2], g[2])), __dmul_rn(g[3], g[3])));
    double qa[4], qb[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) { qa[c] = __ddiv_rn(o[c], no); qb[c] = __ddiv_rn(g[c], ng); }
    const double dot = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(qa[0], qb[0]), __dmul_rn(qa[1], qb[1])), __dmul_rn(qa[2], qb[2])), __dmul_rn(qa[3], qb[3]));
    if (dot < 0.0) {
#pragma unroll
        for (int c = 0; c < 4; ++c) qb[c] = -qb[c];
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) r[c] = __dadd_rn(qa[c], __dmul_rn(w, __dsub_rn(qb[c], qa[c])));
    const double nr = __dsqrt_rn(__dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(r[0], r[0]), __dmul_rn(r[1], r[1])), __dmul_rn(r[2], r[2])), __dmul_rn(r[3], r[3])));
#pragma unroll
    for (int c = 0; c < 4; ++c) r[c] = __ddiv_rn(r[c], nr);
}

template <typename T, bool MOTION = false>
__global__ __launch_bounds__(64) void osc_action_kernel(const typename action_args_of<MOTION>::type a) {
    __shared__ T s_t[64 * IRLOSC_MAX_DEV * 7];      // the wave's target tile
    const int lane = threadIdx.x;
    const int b0 = (int)blockIdx.x * 64;
    const int nvalid = min(64, a.B - b0);           // robots of this wave
    const bool valid = lane < nvalid;
    const size_t so = (size_t)b0 + lane;
    if (a.init) {
        if (valid) list_fresh(a.st, a.stride, so);
        return;
    }
    const int row = a.ndev * 7;
    T* __restrict__ tg = (T*)a.tgt + (size_t)b0 * row;
    tgt_tile_load(s_t, tg, nvalid, row);
    bool moved = false;
    if (valid) {                                    // idle lanes load nothing
        const int A = a.A;
        const double* __restrict__ xs = a.xside + (size_t)blockIdx.x * a.n_entries * 64 + lane;
        T* ta = s_t + lane * row + a.active * 7;
        int act = a.st.action[so];
        const int ent = a.st.entered[so];
        const bool first = ent < 0;                 // the first tick that runs this robot: tick 0, or later behind narrower rollouts
        double err = a.st.err[so];
        double ea[7];
#pragma unroll
        for (int c = 0; c < 7; ++c) ea[c] = xs[(size_t)a.ee_act[c] * 64];
        int stp = 0;                                // MOTION: the robot's step, its goal and origin where this tick enters a WP
        bool wp_entered = false;
        double g[7], og[7];
        if constexpr (MOTION) stp = a.mo.m_step[so];
        if (!first && act < A) {                    // after_step of the previous tick, on the state its plant step produced
            double t7[7], e[6];
#pragma unroll
            for (int c = 0; c < 7; ++c) t7[c] = (double)ta[c];
            task_error6<double>(ea, t7, true, true, e);
            double s2 = __dmul_rn(e[0], e[0]);
#pragma unroll
            for (int c = 1; c < 6; ++c) s2 = __dadd_rn(s2, __dmul_rn(e[c], e[c]));
            err = __dsqrt_rn(s2);
            a.st.err[so] = err;
            bool next;
            if (a.kind[act] == 0) {
                next = err <= a.max_error[act];     // NaN: stays
                if constexpr (MOTION) next = next && (a.steps[act] == 0 || stp == a.steps[act]);      // an INTERP has arrived first
            } else {
                const int gl = a.st.grip_left[so] - 1;
                a.st.grip_left[so] = gl;
                next = gl <= 0;
            }
            if (next) {
                act += 1;
                a.st.action[so] = act;
                if (act == A) a.st.finished_tick[so] = a.tick;
            }
        }
        double sx[3];
        if (first) {
#pragma unroll
            for (int c = 0; c < 3; ++c) a.st.start_xyz[(size_t)c * a.stride + so] = sx[c] = ea[c];
        }
        if (act < A && ent != act) {
            a.st.entered[so] = act;
            a.st.gripper_force[so] = a.force[act];
            if (a.kind[act] == 0) {
                if (a.passive >= 0) {
                    T* tp = s_t + lane * row + a.passive * 7;
#pragma unroll
                    for (int c = 0; c < 7; ++c)
                        if (c < 3 || a.hold) tp[c] = (T)xs[(size_t)a.ee_pas[c] * 64];
                        else tp[c] = (T)a.passive_quat[c - 3];
                }
                const double* __restrict__ p = a.per_robot ? a.table + (((size_t)blockIdx.x * A + act) * 7) * 64 + lane : a.table + (size_t)act * 7;
                const int cs = a.per_robot ? 64 : 1;
                const bool from_start = a.xyz_from_start[act] != 0;
                if (from_start && !first) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) sx[c] = a.st.start_xyz[(size_t)c * a.stride + so];
                }
                const int xo = a.obj_pose ? a.xyz_obj[act] : -1, qo = a.obj_pose ? a.quat_obj[act] : -1;
                if (xo < 0 && qo < 0) {
#pragma unroll
                    for (int c = 0; c < 7; ++c) {
                        if constexpr (MOTION) g[c] = (c < 3 && from_start) ? sx[c < 3 ? c : 0] : p[c * cs];
                        else ta[c] = (c < 3 && from_start) ? (T)sx[c < 3 ? c : 0] : (T)p[c * cs];
                    }
                } else {                            // the table's words are an offset / the grip rotation on the object's pose of this tick
                    double w[7];
#pragma unroll
                    for (int c = 0; c < 7; ++c) w[c] = p[c * cs];
                    if (xo >= 0) {
#pragma unroll
                        for (int c = 0; c < 3; ++c) w[c] = __dadd_rn(a.obj_pose[(size_t)(xo * 7 + c) * a.stride + so], w[c]);
                    }
                    if (qo >= 0) {
                        double q[4];
#pragma unroll
                        for (int c = 0; c < 4; ++c) q[c] = a.obj_pose[(size_t)(qo * 7 + 3 + c) * a.stride + so];
                        const double g[4] = {w[3], w[4], w[5], w[6]};
                        quat_mul_rn(q, g, w + 3);
                    }
#pragma unroll
                    for (int c = 0; c < 7; ++c) {
                        if constexpr (MOTION) g[c] = (c < 3 && from_start) ? sx[c < 3 ? c : 0] : w[c];
                        else ta[c] = (c < 3 && from_start) ? (T)sx[c < 3 ? c : 0] : (T)w[c];
                    }
                }
                err = __builtin_huge_val();
                a.st.err[so] = err;
                if constexpr (MOTION) {
                    const double mean = a.noise_mean[act], sd = a.noise_std[act];
                    if (sd > 0.0 || mean != 0.0) {
                        const uint32_t dr = a.mo.m_draws[so];
                        double z[3];
                        normal3(a.seed, (uint32_t)so, dr, (uint32_t)act, z);
#pragma unroll
                        for (int c = 0; c < 3; ++c) g[c] = __dadd_rn(g[c], __dadd_rn(mean, __dmul_rn(sd, z[c])));
                        a.mo.m_draws[so] = dr + 1u;
                    }
#pragma unroll
                    for (int c = 0; c < 7; ++c) {
                        og[c] = ea[c];
                        a.mo.m_goal[(size_t)c * a.stride + so] = g[c];
                        a.mo.m_origin[(size_t)c * a.stride + so] = og[c];
                    }
                    stp = 0;
                    wp_entered = true;
                    if (a.steps[act] == 0) {        // the WP jumps (an INTERP's step and target: below)
                        a.mo.m_step[so] = 0;
#pragma unroll
                        for (int c = 0; c < 7; ++c) ta[c] = (T)g[c];
                        moved = true;
                    }
                } else {
                    moved = true;
                }
            } else {
                a.st.grip_left[so] = a.grip_ticks[act];
            }
        }
        if constexpr (MOTION) {                     // an INTERP on its way: the entry tick and every later one until step == N
            const int N = (act < A && a.kind[act] == 0) ? a.steps[act] : 0;
            if (N >= 1 && stp < N) {
                if (!wp_entered) {
#pragma unroll
                    for (int c = 0; c < 7; ++c) {
                        g[c] = a.mo.m_goal[(size_t)c * a.stride + so];
                        og[c] = a.mo.m_origin[(size_t)c * a.stride + so];
                    }
                }
                stp += 1;
                a.mo.m_step[so] = stp;
                if (stp < N) {
                    const double w = __ddiv_rn((double)stp, (double)N);
                    double q[4];
                    quat_nlerp_rn(og + 3, g + 3, w, q);
#pragma unroll
                    for (int c = 0; c < 3; ++c) ta[c] = (T)__dadd_rn(og[c], __dmul_rn(w, __dsub_rn(g[c], og[c])));
#pragma unroll
                    for (int c = 0; c < 4; ++c) ta[3 + c] = (T)q[c];
                } else {
#pragma unroll
                    for (int c = 0; c < 7; ++c) ta[c] = (T)g[c];
                }
                moved = true;
            }
        }
        if (act < A && a.kind[act] == 0) {          // the error-adaptive velocity limit of the active arm (insertion_task.py:293-295)
            const double v = __dmul_rn(a.kp[act], err);
            double m = v < a.max_speed[act] ? v : a.max_speed[act];          // min(max_speed, v) as the host evaluates it
            m = m > a.min_speed[act] ? m : a.min_speed[act];                 // max(min_speed, m)
            a.st.max_vel0[so] = m;
            ((T*)a.gains)[(so * a.ndev + a.active) * IRLOSC_GAIN_WORDS + 9] = (T)m;
        }
    }
    tgt_tile_store(tg, s_t, nvalid, row, moved);
}

}  // namespace irlosc
