// The EPISODE LOG of a rollout (irlosc_rollout_from_q_logged): on a logged tick, the channels the caller asked for of the robots it asked
// for, gathered into one SAMPLE of the context's device ring -- per channel a dense row-major plane [R][w] of doubles, the planes in
// ascending bit order (irlosc_log_layout).  The kernel only reads the tick's state; nothing the tick computes depends on it.  Two launches
// of one kernel per logged tick, told apart by the channel mask:
//
//   FRONT, directly behind the give-up pass and in front of the waypoint cycler: QPOS, QVEL (the slot's row-major coordinates, which the
//       plant has not advanced yet: what the tick's walk read), EE_POSE (the walk's poses in the tick's exchange block), TARGETS and WRENCH
//       (as the OSC step read them: a list's or a stream's targets of the tick are in, the cycler's move is not), U (the give-up pass has
//       run: every robot has its torques), FLAGS (the step's word; what the plant adds behind it is not in), OBJECT_POSE (the action
//       objects as this tick's object kernel left them: seven pose words and the holder as a double, per object), POLICY_OUT and
//       POLICY_SAMPLE (the out, act and logp planes of the policy's per-robot state as this tick's policy kernel left them), REWARD (r, ret,
//       steps and goal_step >= 0 of the reward's per-robot state as this tick's reward kernel, the launch in front of this one, left them).
//   BACK, behind the joint rows and directly in front of the plant: WALL_FORCE and JOINT_TAU, the `force` and `tau` planes of the walls'
//       and rows' per-robot state as this tick's APPLY launches left them.  Launched only where one of the two is asked for.
//
// One block of 64 lanes per 64 LOGGED robots; lane l of block g logs robot g 64 + l, or robots[g 64 + l] with an index list.  A block
// owns 64 w consecutive doubles of every plane (channel-major on purpose: the plant's row-major tiles), so every store is one of a
// coalesced tile, a ragged last block's tile short by its idle lanes' rows.
//   row-major sources (qpos, qvel, u, targets, wrench, flags), all robots logged: the block's nvalid w consecutive source words are
//       loaded coalesced, widened and stored -- a tile copy, no LDS;
//   with an index list each lane gathers its robot's w words into its row of an LDS tile, and the tile is stored as above;
//   walk-layout sources (EE poses in the exchange block [wave][entry][64], the state planes [plane][stride] of walls and rows): one
//       coalesced load per entry across the lanes into the LDS tile's column, then the tile is stored as above (osc_plant.hpp's u tile
//       the other way round).
// The LDS tile is 64 x the widest channel of the launch (k13: 64 x 25 doubles = 12.8 KB), dynamic.  Widths and the mask are kernel
// arguments, uniform over the launch: every branch and every barrier is uniform, loops over a runtime width only move addresses (no
// per-lane array, no scratch) and are unrolled by eight, so that eight independent loads are in flight where a launch of a few blocks (a
// short robot list) would otherwise pay every load's latency in turn.  Widening float32 words and the uint32 flags to double is exact; a NaN keeps its payload bits' upper part
// and its sign (float64 sources are copied bit for bit).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/irlosc.h"

namespace irlosc {

constexpr int LOG_CHANNELS = 13;
constexpr uint32_t LOG_FRONT = IRLOSC_LOG_QPOS | IRLOSC_LOG_QVEL | IRLOSC_LOG_EE_POSE | IRLOSC_LOG_TARGETS | IRLOSC_LOG_WRENCH |
                               IRLOSC_LOG_U | IRLOSC_LOG_FLAGS | IRLOSC_LOG_OBJECT_POSE | IRLOSC_LOG_POLICY_OUT | IRLOSC_LOG_POLICY_SAMPLE | IRLOSC_LOG_REWARD;
constexpr uint32_t LOG_BACK = IRLOSC_LOG_WALL_FORCE | IRLOSC_LOG_JOINT_TAU;

// Words per robot of channel bit i (nobj: the action objects of the slot; 0: it has none, and no OBJECT_POSE channel; n_out: the outputs
// of its policy; 0: it has none, and neither POLICY channel; bit 12, REWARD, is four words wherever a slot knows it)
__host__ __device__ inline int log_width(int i, int n, int ndev, int nobj = 0, int n_out = 0) {
    return i == 12 ? 4 : i == 10 ? n_out : i == 11 ? n_out + 1 : i == 9 ? nobj * 8 : i == 0 || i == 1 || i == 5 || i == 8 ? n : i == 2 || i == 3 ? ndev * 7 : i == 4 ? ndev * 6 : i == 6 ? 1 : ndev * 3;
}

struct LogArgs {
    double* sample;                   // the sample of this tick in the ring
    int64_t off[LOG_CHANNELS];        // offset of each channel's plane inside it, in doubles (irlosc_log_layout)
    const int32_t* robots;            // [R] strictly ascending in [0, B), or nullptr: robots 0 .. R - 1
    const double* qpos;               // [B][n] row-major
    const double* qvel;
    const double* xside;              // the tick's exchange block [walk wave][n_entries][64]
    const void* tgt;                  // [B][ndev][7], record type
    const void* wrench;               // [B][ndev][6], record type: the feed's wrench of the tick
    const void* u;                    // [B][n], record type
    const uint32_t* flags;            // [B]
    const double* wall_force;         // [3][ndev][stride]
    const double* joint_tau;          // [n][stride]
    const double* obj_pose;           // [IRLOSC_MAX_OBJECTS 7][stride] the action objects' poses (osc_object.hpp) ...
    const int32_t* obj_holder;        // [IRLOSC_MAX_OBJECTS][stride] ... and their holders
    const float* po_out;              // [n_out][stride] the policy's output (with a Gaussian head: the mean) ...
    const float* po_act;              // [n_out][stride] ... the sampled action ...
    const double* po_logp;            // [stride] ... and its log-probability (osc_policy.hpp: PolicyState)
    const double* rw_r;               // [stride] the reward's r, ret ...
    const double* rw_ret;
    const int32_t* rw_steps;          // [stride] ... steps and goal_step (osc_reward.hpp: RewardState)
    const int32_t* rw_goal_step;
    uint32_t mask;                    // the channels of THIS launch
    int32_t R, n, ndev, n_entries, stride, nobj, n_out;
    int32_t ee0[IRLOSC_MAX_DEV];      // exchange entry of each device's EE pose (x y z qw qx qy qz follow each other)
};

template <typename T>
__global__ __launch_bounds__(64) void osc_log_kernel(const LogArgs a) {
    extern __shared__ double s_t[];                 // [64][w] of the channel in hand
    const int lane = threadIdx.x;
    const int r0 = (int)blockIdx.x * 64;
    const int nvalid = min(64, a.R - r0);           // logged robots of this block (a ragged last block: its idle lanes store nothing)
    const bool valid = lane < nvalid;
    const bool listed = a.robots != nullptr;
    const int rb = !valid ? 0 : listed ? a.robots[r0 + lane] : r0 + lane;      // the robot this lane logs
    const size_t wave = (size_t)(rb >> 6);
    const int wl = rb & 63;

    // the block's tile of a plane: nvalid w consecutive doubles from LDS
    auto store_tile = [&](int ch, int w) {
        __syncthreads();
        double* __restrict__ out = a.sample + a.off[ch] + (size_t)r0 * w;
#pragma unroll 8
        for (int idx = lane; idx < nvalid * w; idx += 64) out[idx] = s_t[idx];
        __syncthreads();
    };
    // a row-major source [B][w] of S
    auto row_major = [&](int ch, int w, const auto* __restrict__ src) {
        if (!listed) {
            double* __restrict__ out = a.sample + a.off[ch] + (size_t)r0 * w;
            const auto* __restrict__ in = src + (size_t)r0 * w;
#pragma unroll 8
            for (int idx = lane; idx < nvalid * w; idx += 64) out[idx] = (double)in[idx];
        } else {
            if (valid) {
#pragma unroll 8
                for (int j = 0; j < w; ++j) s_t[lane * w + j] = (double)src[(size_t)rb * w + j];
            }
            store_tile(ch, w);
        }
    };
    if (a.mask & IRLOSC_LOG_QPOS) row_major(0, a.n, a.qpos);
    if (a.mask & IRLOSC_LOG_QVEL) row_major(1, a.n, a.qvel);
    if (a.mask & IRLOSC_LOG_EE_POSE) {
        const int w = a.ndev * 7;
        const double* __restrict__ col = a.xside + wave * (size_t)a.n_entries * 64 + wl;
        if (valid)
            for (int d = 0; d < a.ndev; ++d)
#pragma unroll
                for (int c = 0; c < 7; ++c) s_t[lane * w + d * 7 + c] = col[(size_t)(a.ee0[d] + c) * 64];
        store_tile(2, w);
    }
    if (a.mask & IRLOSC_LOG_TARGETS) row_major(3, a.ndev * 7, (const T*)a.tgt);
    if (a.mask & IRLOSC_LOG_WRENCH) row_major(4, a.ndev * 6, (const T*)a.wrench);
    if (a.mask & IRLOSC_LOG_U) row_major(5, a.n, (const T*)a.u);
    if (a.mask & IRLOSC_LOG_FLAGS) row_major(6, 1, a.flags);
    if (a.mask & IRLOSC_LOG_WALL_FORCE) {
        const int w = a.ndev * 3;
        const size_t plane = (size_t)a.ndev * a.stride;
        if (valid)
            for (int d = 0; d < a.ndev; ++d)
#pragma unroll
                for (int c = 0; c < 3; ++c) s_t[lane * w + d * 3 + c] = a.wall_force[c * plane + (size_t)d * a.stride + rb];
        store_tile(7, w);
    }
    if (a.mask & IRLOSC_LOG_JOINT_TAU) {
        const int w = a.n;
        if (valid) {
#pragma unroll 8
            for (int j = 0; j < w; ++j) s_t[lane * w + j] = a.joint_tau[(size_t)j * a.stride + rb];
        }
        store_tile(8, w);
    }
    if (a.mask & IRLOSC_LOG_OBJECT_POSE) {
        const int w = a.nobj * 8;
        if (valid)
            for (int o = 0; o < a.nobj; ++o) {
#pragma unroll
                for (int c = 0; c < 7; ++c) s_t[lane * w + o * 8 + c] = a.obj_pose[(size_t)(o * 7 + c) * a.stride + rb];
                s_t[lane * w + o * 8 + 7] = (double)a.obj_holder[(size_t)o * a.stride + rb];
            }
        store_tile(9, w);
    }
    if (a.mask & IRLOSC_LOG_POLICY_OUT) {
        const int w = a.n_out;
        if (valid) {
#pragma unroll 8
            for (int j = 0; j < w; ++j) s_t[lane * w + j] = (double)a.po_out[(size_t)j * a.stride + rb];
        }
        store_tile(10, w);
    }
    if (a.mask & IRLOSC_LOG_POLICY_SAMPLE) {
        const int w = a.n_out + 1;
        if (valid) {
#pragma unroll 8
            for (int j = 0; j < a.n_out; ++j) s_t[lane * w + j] = (double)a.po_act[(size_t)j * a.stride + rb];
            s_t[lane * w + a.n_out] = a.po_logp[rb];
        }
        store_tile(11, w);
    }
    if (a.mask & IRLOSC_LOG_REWARD) {
        if (valid) {
            s_t[lane * 4] = a.rw_r[rb];
            s_t[lane * 4 + 1] = a.rw_ret[rb];
            s_t[lane * 4 + 2] = (double)a.rw_steps[rb];
            s_t[lane * 4 + 3] = a.rw_goal_step[rb] >= 0 ? 1.0 : 0.0;
        }
        store_tile(12, 4);
    }
}

}  // namespace irlosc
