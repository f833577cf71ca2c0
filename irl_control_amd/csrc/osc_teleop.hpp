// The TELEOPERATION STREAM of a rollout (irlosc_set_teleop_stream): per tick and robot the space-mouse demo's caller loop
// (examples/teleop_loops.py::space_mouse_loop on input_devices/space_mouse.py::SpaceMouse.update_state) -- integrate the tick's rate
// reading into the 6-DoF plate pose, derive the followers' targets from it and write them -- so that the OSC step of the SAME tick
// aims at them without the host in between.  It runs where the action list's kernel runs, between the walk (and the sensor feed's
// wrench) and the first OSC kernel of the tick: the reference calls update_state() and then generate() on one tick.
//
// One lane per robot, one block per walk wave (its 64 robots), like the action kernel.  The target record tgt[B][ndev][7] goes through
// the wave's target tile (osc_common.hpp: its contract); a tick writes the listed devices of every robot, so every wave with a robot
// stores its tile.  The pose is SoA [6][stride] (x y z roll pitch yaw).  Per-robot readings are [walk wave][T * 6][64]: six coalesced
// 512-byte lines per wave and tick; a shared stream's six readings of the tick and the follower table are kernel arguments.  Nothing
// of the exchange block is read.  The arithmetic is float64 whatever the record type, every product and sum rounded on its own and in
// the order written here: but for sin / cos / atan2 the host can repeat it bit for bit (irl_control_amd/teleop.py::stream_step).
//
// Per robot on a tick with reading r (inc = increment):
//   x += inc r0;  y += inc r1;  z += inc r2;  yaw = wrap(yaw - inc r5);  pitch = wrap(pitch - inc r4);  roll = wrap(roll + inc r3)
//   q_p = qx(pitch) (x) qy(roll) (x) qz(yaw)      (euler2quat(pitch, roll, yaw, 'rxyz'): pitch and roll swapped, as in the reference)
//   RIGID d:    tgt xyz = p + R(q_p) off_xyz[d];  tgt quat = q_p (x) off_quat[d]
//   HEADING d:  h = atan2(y, x) + heading_offset[d];  tgt quat = (cos(h / 2), 0, 0, sin(h / 2));  xyz stays
//
// The per-robot body -- reading -> pose -> followers' targets -- is teleop_follow: the policy kernel (osc_policy.hpp) calls it on the reading its
// network computed, and its setter uses this kernel's init launch.
//
// init = 1 (irlosc_set_teleop_stream): pose = origin (per robot: [walk wave][6][64] at `readings`; shared: `r`); no target is touched.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/irlosc.h"
#include "osc_common.hpp"

namespace irlosc {

struct PlateState { double* pose; };      // the stream's per-robot state (and a policy's), the plate: [6][stride], x y z roll pitch yaw
// One robot's fresh plate (so: its column) at the origin given: the init launch of irlosc_set_teleop_stream and irlosc_set_policy, a reset of episodes
__device__ __forceinline__ void plate_fresh(PlateState st, int stride, size_t so, const double origin[6]) {
#pragma unroll
    for (int c = 0; c < 6; ++c) st.pose[(size_t)c * stride + so] = origin[c];
}

struct TeleopArgs {
    void* tgt;                // [B][ndev][7] targets of the slot, record type
    PlateState st;
    const double* readings;   // per_robot: [walk wave][T * 6][64] (init: the origins [walk wave][6][64]); else not read
    double r[6];              // !per_robot: the tick's reading (init: the origin)
    double inc;
    double off_xyz[IRLOSC_MAX_DEV][3], off_quat[IRLOSC_MAX_DEV][4], heading[IRLOSC_MAX_DEV];
    int32_t kind[IRLOSC_MAX_DEV];
    int32_t B, ndev, stride, T, per_robot, index, init;      // index: of the tick's reading in [0, T)
};

__device__ __forceinline__ double teleop_wrap(double a) { return atan2(sin(a), cos(a)); }

// One robot's tick on reading r: the pose integrated and stored, the followers' targets written into the robot's row of the wave's
// target tile s_t (`row` words per robot).  The body of the stream's tick; osc_policy.hpp calls it with the reading its network computed.
template <typename T>
__device__ __forceinline__ void teleop_follow(const TeleopArgs& a, T* s_t, int lane, size_t so, int row, const double r[6]) {
    double p[6];
#pragma unroll
    for (int c = 0; c < 6; ++c) p[c] = a.st.pose[(size_t)c * a.stride + so];
#pragma unroll
    for (int c = 0; c < 3; ++c) p[c] = __dadd_rn(p[c], __dmul_rn(a.inc, r[c]));
    p[5] = teleop_wrap(__dsub_rn(p[5], __dmul_rn(a.inc, r[5])));
    p[4] = teleop_wrap(__dsub_rn(p[4], __dmul_rn(a.inc, r[4])));
    p[3] = teleop_wrap(__dadd_rn(p[3], __dmul_rn(a.inc, r[3])));
#pragma unroll
    for (int c = 0; c < 6; ++c) a.st.pose[(size_t)c * a.stride + so] = p[c];
    // q_p = qx(pitch) (x) qy(roll) (x) qz(yaw)
    const double hx = __dmul_rn(p[4], 0.5), hy = __dmul_rn(p[3], 0.5), hz = __dmul_rn(p[5], 0.5);
    const double cx = cos(hx), sx = sin(hx), cy = cos(hy), sy = sin(hy), cz = cos(hz), sz = sin(hz);
    const double cc = __dmul_rn(cy, cz), ss = __dmul_rn(sy, sz), sc = __dmul_rn(sy, cz), cs = __dmul_rn(cy, sz);
    const double qw = __dsub_rn(__dmul_rn(cx, cc), __dmul_rn(sx, ss)), qx = __dadd_rn(__dmul_rn(cx, ss), __dmul_rn(sx, cc));
    const double qy = __dsub_rn(__dmul_rn(cx, sc), __dmul_rn(sx, cs)), qz = __dadd_rn(__dmul_rn(cx, cs), __dmul_rn(sx, sc));
    // R(q_p): transforms.quat2mat (|q_p| is 1 to rounding, far from its Nq < eps branch)
    const double qp[4] = {qw, qx, qy, qz};
    double R[3][3];
    quat2mat_rn(qp, R);
    for (int d = 0; d < a.ndev; ++d) {
        T* t = s_t + lane * row + d * 7;
        if (a.kind[d] == IRLOSC_TELEOP_RIGID) {
            double ro[3], qt[4];
            mat_vec_rn(R, a.off_xyz[d], ro);
            quat_mul_rn(qp, a.off_quat[d], qt);
#pragma unroll
            for (int c = 0; c < 3; ++c) t[c] = (T)__dadd_rn(p[c], ro[c]);
#pragma unroll
            for (int c = 0; c < 4; ++c) t[3 + c] = (T)qt[c];
        } else if (a.kind[d] == IRLOSC_TELEOP_HEADING) {
            const double h = __dmul_rn(__dadd_rn(atan2(p[1], p[0]), a.heading[d]), 0.5);
            t[3] = (T)cos(h); t[4] = (T)0.0; t[5] = (T)0.0; t[6] = (T)sin(h);
        }
    }
}

template <typename T>
__global__ __launch_bounds__(64) void osc_teleop_kernel(const TeleopArgs a) {
    __shared__ T s_t[64 * IRLOSC_MAX_DEV * 7];      // the wave's target tile
    const int lane = threadIdx.x;
    const int b0 = (int)blockIdx.x * 64;
    const int nvalid = min(64, a.B - b0);           // robots of this wave
    const bool valid = lane < nvalid;
    const size_t so = (size_t)b0 + lane;
    const int E = a.init ? 6 : a.T * 6;             // entries per robot of the table at `readings`
    double r[6];
    if (valid) {                                    // idle lanes load nothing
        const size_t e0 = ((size_t)blockIdx.x * E + (a.init ? 0 : (size_t)a.index * 6)) * 64 + lane;
#pragma unroll
        for (int c = 0; c < 6; ++c) r[c] = a.per_robot ? a.readings[e0 + (size_t)c * 64] : a.r[c];
    }
    if (a.init) {
        if (valid) plate_fresh(a.st, a.stride, so, r);
        return;
    }
    const int row = a.ndev * 7;
    T* __restrict__ tg = (T*)a.tgt + (size_t)b0 * row;
    tgt_tile_load(s_t, tg, nvalid, row);
    if (valid) teleop_follow(a, s_t, lane, so, row, r);
    tgt_tile_store(tg, s_t, nvalid, row, valid);
}

}  // namespace irlosc
