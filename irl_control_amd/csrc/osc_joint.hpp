// JOINT ROWS of a rollout (irlosc_set_joints): the joint-space forces of the scene that the plant lacks -- the hinges' range stops, the
// equality rows that tie a Robotiq finger linkage to its driven knuckle, and the gripper motors -- as one torque per hinge, computed from
// that hinge's own coordinates and taken off the bias in front of the unchanged plant kernel.  One launch per tick (APPLY; there is no
// SENSE half: these forces act inside the gripper or at arm hinges, not at the F/T site frame, and the feed's wrench does not see them),
// behind the give-up pass, the waypoint cycler, the pushes' APPLY and the walls' APPLY, directly in front of the plant.
//
// Row r (kind, hinge a, hinge b, eight doubles of table), q / qd = this tick's coordinates, which the plant has not advanced yet:
//   LIMIT   hinge a, row  lo hi k c 0 0 0 0   (lo < hi, k >= 0, c >= 0)
//       g_lo = lo - q,  f_lo = k g_lo - c qd,  t_lo = (g_lo > 0 && f_lo > 0) ? f_lo : 0
//       g_hi = q - hi,  f_hi = k g_hi + c qd,  t_hi = (g_hi > 0 && f_hi > 0) ? f_hi : 0
//       contribution to hinge a:  t_lo - t_hi          (a stop never pulls; a NaN: no contact, no force)
//   COUPLE  hinges a and b, row  a0 a1 qa0 qb0 k c 0 0 -- an <equality><joint joint1 joint2 polycoef> row of the scene, LINEAR only.
//       Hinge a is MuJoCo's joint1, the DEPENDENT y; hinge b is joint2, the x:  y - y0 = a0 + a1 (x - x0).  (This reading of joint1 /
//       joint2 follows MuJoCo's documentation.  Nobody has compared it with MuJoCo on this project: MuJoCo is not installed.)
//       e = (q_a - qa0) - (a0 + a1 (q_b - qb0)),   de = qd_a - a1 qd_b,   f = k e + c de
//       contribution to hinge a:  -f,   to hinge b:  a1 f      (f, or a1 f, not finite: that contribution is nothing)
//   DRIVE   hinge a, row  gear value 0 0 0 0 0 0, source CONST: ctrl = value;  source ACTION: ctrl is per-robot state held across ticks,
//       initially 0, and on a tick where the slot has an action list in force whose active device is the row's device and the robot's
//       gripper_force state (osc_action.hpp, which has run on this tick already) is non-zero, ctrl = gripper_force -- the reference's
//       `if gripper_force: ctrl[idx] = gripper_force`: a later action with force 0.0 keeps the grip.
//       contribution to hinge a:  gear ctrl            (ctrl or the product not finite: nothing)
// Float64 whatever the record type; every product, add and subtract rounded on its own, nothing contracted, sums left to right: the host
// can repeat it bit for bit (joints.py).
//
// ACCUMULATION ORDER.  tau_j is the sum of the contributions to hinge j in ASCENDING ROW INDEX, the first taken as it is (a COUPLE row
// contributes once to its hinge a and once to its hinge b).  The kernel walks the hinges, not the rows: the host hands it, per hinge j,
// the items (row, role) that name j, sorted by row (JointArgs::first / item), so a lane carries ONE accumulator and no per-lane tau[NJ]
// indexed at run time (which would live in scratch).  A COUPLE row is evaluated at both of its hinges from the same operands, so both
// see the same f; its per-row state is written where it is evaluated as hinge a.  Then, where tau_j != 0,
//       bias_j = bias_j - tau_j        in place on the tick's exchange block (nothing is stored where tau_j is zero: a -0.0 bias stays)
// so that the plant integrates M^-1 (u - bias - damping qvel + tau) untouched.  Nothing between the walk and the plant writes the bias
// but the pushes' and walls' APPLY ahead of this kernel.
//
// One lane per robot, one block per walk wave (its 64 robots).  Hinge and row indices are kernel arguments, uniform over the launch:
// FeTopo<TOPO>::bias_index(0) + j is contiguous in j (as osc_plant.hpp reads it) and qt's entries are 2 j, 2 j + 1, so a runtime j only
// moves an address.  A shared table [R][8] is read with scalar loads, a per-robot one [walk wave][R 8][64] one coalesced 512-byte line
// per operand.  State is SoA with stride max_batch: tau[NJ][stride] (what the last tick applied, zeros included),
// max_violation[R][stride] (the largest g > 0 of a LIMIT, |e| of a COUPLE, 0 of a DRIVE), active_ticks[R][stride] (ticks with a
// non-zero contribution of the row), ctrl[R][stride] (DRIVE rows).  No LDS, no barrier.  Idle lanes of a ragged last wave neither load
// nor store.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/irlosc.h"
#include "osc_frontend_lane.hpp"

namespace irlosc {

struct JointState {                 // the rows' per-robot state
    double* tau;                    // [NJ][stride]
    double* max_violation; double* ctrl; int32_t* active_ticks;      // [R][stride] each
};
// One robot's fresh state of R rows (b: its column): the fills of irlosc_set_joints, written by a reset of episodes (ctrl = 0: an ACTION drive lets go)
template <int NJ>
__device__ __forceinline__ void joint_fresh(JointState st, int R, int stride, size_t b) {
#pragma unroll
    for (int j = 0; j < NJ; ++j) st.tau[(size_t)j * stride + b] = 0.0;
    for (int r = 0; r < R; ++r) { const size_t o = (size_t)r * stride + b; st.max_violation[o] = 0.0; st.ctrl[o] = 0.0; st.active_ticks[o] = 0; }
}

struct JointArgs {
    double* xside;                  // the tick's exchange block [walk wave][n_compact][64], bias entries in place
    const double* qt;               // the slot's coordinates in the walk's layout [walk wave][2 NJ][64]
    const double* table;            // per_robot: [walk wave][R][8][64], else [R][8]
    const double* gripper_force;    // the action state's gripper_force[stride] of the list in force, or nullptr (no list)
    JointState st;
    uint64_t armed;                 // bit r: row r is an ACTION drive whose device is the active device of the list in force
    int32_t B, R, per_robot, stride;
    uint8_t kind[IRLOSC_MAX_JOINT_ROWS], ja[IRLOSC_MAX_JOINT_ROWS], jb[IRLOSC_MAX_JOINT_ROWS], source[IRLOSC_MAX_JOINT_ROWS];
    uint8_t first[IRLOSC_MAX_N + 1];             // items first[j] .. first[j + 1] - 1 name hinge j, in ascending row
    uint8_t item[2 * IRLOSC_MAX_JOINT_ROWS];     // row | 0x80: the row's hinge b (a COUPLE), else its hinge a
};

template <class TOPO>
__global__ __launch_bounds__(64) void osc_joint_kernel(const JointArgs a) {
    using TI = FeTopo<TOPO>;
    constexpr int n_compact = TI::n_compact();
    constexpr int NJ = TOPO::NJ;
    constexpr int bias0 = TI::bias_index(0);
    constexpr double DMAX = 1.7976931348623157e308;
    const int lane = threadIdx.x;
    const int b = (int)blockIdx.x * 64 + lane;
    if (b >= a.B) return;                           // (no barrier below)
    const double* __restrict__ tab = a.per_robot ? a.table + (size_t)blockIdx.x * a.R * 8 * 64 + lane : a.table;
    const int cs = a.per_robot ? 64 : 1;
    double* col = a.xside + (size_t)blockIdx.x * n_compact * 64 + lane;
    const double* __restrict__ gq = a.qt + (size_t)blockIdx.x * (2 * NJ * 64) + lane;
#pragma nounroll
    for (int j = 0; j < NJ; ++j) {                  // (every index and condition below uniform over the launch: kernel arguments)
        double tau = 0.0;
        const int i1 = a.first[j + 1];
#pragma nounroll
        for (int i = a.first[j]; i < i1; ++i) {
            const int r = a.item[i] & 0x7f;
            const bool as_b = (a.item[i] & 0x80) != 0;
            const int kind = a.kind[r];
            const double* __restrict__ row = tab + (size_t)r * 8 * cs;
            const size_t so = (size_t)r * a.stride + b;
            double t;                               // the row's contribution to hinge j
            if (kind == IRLOSC_JOINT_LIMIT) {
                const double q = gq[(size_t)(2 * j) * 64], qd = gq[(size_t)(2 * j + 1) * 64];
                const double lo = row[0], hi = row[cs], k = row[2 * cs], c = row[3 * cs];
                const double g_lo = __dsub_rn(lo, q), g_hi = __dsub_rn(q, hi);
                const double cqd = __dmul_rn(c, qd);
                const double f_lo = __dsub_rn(__dmul_rn(k, g_lo), cqd), f_hi = __dadd_rn(__dmul_rn(k, g_hi), cqd);
                const double t_lo = (g_lo > 0.0 && f_lo > 0.0) ? f_lo : 0.0;      // NaN: no contact
                const double t_hi = (g_hi > 0.0 && f_hi > 0.0) ? f_hi : 0.0;
                t = __dsub_rn(t_lo, t_hi);
                const double g = g_lo > g_hi ? g_lo : g_hi;
                if (g > 0.0 && g > a.st.max_violation[so]) a.st.max_violation[so] = g;
                if (t != 0.0) a.st.active_ticks[so] += 1;
            } else if (kind == IRLOSC_JOINT_COUPLE) {
                const int ha = a.ja[r], hb = a.jb[r];
                const double qa = gq[(size_t)(2 * ha) * 64], qda = gq[(size_t)(2 * ha + 1) * 64];
                const double qb = gq[(size_t)(2 * hb) * 64], qdb = gq[(size_t)(2 * hb + 1) * 64];
                const double a0 = row[0], a1 = row[cs], qa0 = row[2 * cs], qb0 = row[3 * cs], k = row[4 * cs], c = row[5 * cs];
                const double e = __dsub_rn(__dsub_rn(qa, qa0), __dadd_rn(a0, __dmul_rn(a1, __dsub_rn(qb, qb0))));
                const double de = __dsub_rn(qda, __dmul_rn(a1, qdb));
                const double f = __dadd_rn(__dmul_rn(k, e), __dmul_rn(c, de));
                const bool ok = fabs(f) <= DMAX;
                if (as_b) {
                    const double p = __dmul_rn(a1, f);
                    t = (ok && fabs(p) <= DMAX) ? p : 0.0;
                } else {
                    t = ok ? -f : 0.0;
                    if (fabs(e) > a.st.max_violation[so]) a.st.max_violation[so] = fabs(e);
                    if (ok && f != 0.0) a.st.active_ticks[so] += 1;
                }
            } else {                                // IRLOSC_JOINT_DRIVE
                const double gear = row[0];
                double ctrl;
                if (a.source[r] == IRLOSC_JOINT_SRC_CONST) ctrl = row[cs];
                else {
                    ctrl = a.st.ctrl[so];
                    if ((a.armed >> r) & 1u) {
                        const double gf = a.gripper_force[b];
                        if (gf != 0.0) ctrl = gf;
                    }
                }
                a.st.ctrl[so] = ctrl;
                const double p = __dmul_rn(gear, ctrl);
                t = (fabs(ctrl) <= DMAX && fabs(p) <= DMAX) ? p : 0.0;
                if (t != 0.0) a.st.active_ticks[so] += 1;
            }
            tau = i == a.first[j] ? t : __dadd_rn(tau, t);
        }
        a.st.tau[(size_t)j * a.stride + b] = tau;
        if (tau != 0.0) {
            double* bj = col + (size_t)(bias0 + j) * 64;
            *bj = __dsub_rn(*bj, tau);
        }
    }
}

}  // namespace irlosc
