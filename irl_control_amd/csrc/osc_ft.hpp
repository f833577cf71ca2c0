// F/T sensor feed of the from-q path (irlosc_set_ft_sensors / irlosc_set_sensordata / irlosc_step_from_q_device): the admittance
// wrench of every robot, rotated into the world by its F/T site frame, from the EE pose the step's own front end computed.
//
// What the reference does per device and tick (irl_control/device.py:135-170, osc.py:179-185): R = site_xmat of ft_frame_<device>,
// force = R sensordata[f0 .. f0 + 3], torque = R sensordata[t0 .. t0 + 3].  The site sits on a body welded to the device's EE body, so
// R = R(ee_quat) R_rel with a constant R_rel = R(ee)^T R(site) (host, irlosc_set_ft_sensors): one 3 x 3 product per device and robot.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/irlosc.h"

namespace irlosc {

constexpr int FT_TRAIN = 8;      // steps per launch: those of a train (R16_TRAIN, checked in irlosc.hip)

// One step of a train whose slot has a sensor feed
struct FtStep {
    const double* sens;       // [B][n_sensor] sensordata
    void* wrench;             // [B][ndev][6] out, record type
    const double* xside;      // fused path: the step's exchange buffer [walk wave][n_entries][64 robots]; nullptr: ee below
    const void* ee;           // path through dense records: ee_pose [B][ndev][7], record type
};

struct FtTrain {
    FtStep s[FT_TRAIN];
    double R[IRLOSC_MAX_DEV][9];          // R_rel[d], row-major
    int32_t f0[IRLOSC_MAX_DEV];           // first sensordata index of the force / torque triple; f0 < 0: no sensor (zero wrench)
    int32_t t0[IRLOSC_MAX_DEV];
    int32_t qe[IRLOSC_MAX_DEV];           // exchange entry of the EE's qw (qx qy qz follow: FeCompactTables::eetab[d][3 .. 6])
    int32_t B, ndev, n_sensor, n_entries;
};

// Lane = robot, blockIdx.y = step.  Loads of the quaternions are coalesced on the fused path (one 512-byte line per entry and wave).
template <typename T>
__global__ __launch_bounds__(64) void osc_ft_wrench_kernel(const FtTrain tr) {
    const int lane = threadIdx.x;
    const int b = (int)blockIdx.x * 64 + lane;
    if (b >= tr.B) return;
    const FtStep& s = tr.s[blockIdx.y];
    const double* sens = s.sens + (size_t)b * tr.n_sensor;
    T* w = (T*)s.wrench + (size_t)b * tr.ndev * 6;
    for (int d = 0; d < tr.ndev; ++d) {
        if (tr.f0[d] < 0) {
#pragma unroll
            for (int i = 0; i < 6; ++i) w[d * 6 + i] = (T)0;
            continue;
        }
        double q[4];
        if (s.xside) {
            const double* x = s.xside + ((size_t)blockIdx.x * tr.n_entries + tr.qe[d]) * 64 + lane;
#pragma unroll
            for (int i = 0; i < 4; ++i) q[i] = x[i * 64];
        } else {
            const T* e = (const T*)s.ee + ((size_t)b * tr.ndev + d) * 7 + 3;
#pragma unroll
            for (int i = 0; i < 4; ++i) q[i] = (double)e[i];
        }
        const double qw = q[0], qx = q[1], qy = q[2], qz = q[3];
        const double E[9] = {1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - qw * qz), 2 * (qx * qz + qw * qy),
                             2 * (qx * qy + qw * qz), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - qw * qx),
                             2 * (qx * qz - qw * qy), 2 * (qy * qz + qw * qx), 1 - 2 * (qx * qx + qy * qy)};
        double S[9];      // site frame in the world: R(ee) R_rel
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c)
                S[r * 3 + c] = E[r * 3] * tr.R[d][c] + E[r * 3 + 1] * tr.R[d][3 + c] + E[r * 3 + 2] * tr.R[d][6 + c];
        const double f[3] = {sens[tr.f0[d]], sens[tr.f0[d] + 1], sens[tr.f0[d] + 2]};
        const double t[3] = {sens[tr.t0[d]], sens[tr.t0[d] + 1], sens[tr.t0[d] + 2]};
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            w[d * 6 + r] = (T)(S[r * 3] * f[0] + S[r * 3 + 1] * f[1] + S[r * 3 + 2] * f[2]);
            w[d * 6 + 3 + r] = (T)(S[r * 3] * t[0] + S[r * 3 + 1] * t[1] + S[r * 3 + 2] * t[2]);
        }
    }
}

}  // namespace irlosc
