// The REWARD of a rollout (irlosc_set_reward): per tick and robot a short list of weighted terms over the state the tick observed and the
// action the tick took, accumulated per episode, plain and discounted, with an optional GOAL that an episode can end on.  It runs behind
// the give-up pass (u is complete there) and directly in front of log FRONT, which can then log it -- so in front of the cycler, which
// moves the targets, and of the plant, which moves the coordinates: r_t = R(the state tick t observed, the action tick t took), and what
// the action does shows in r_{t+1}.  The kernel only reads the tick's state and writes its own.
//
// One lane per robot, one block per walk wave (its 64 robots), like the other program kernels.  The term list, the point kinds and the
// goal travel as uniform launch arguments: every branch below is uniform over the launch, and a loop over the terms only picks addresses
// (no per-lane array with a run-time index, no scratch).  Operands:
//   EE poses (the tick's exchange block [walk wave][entry][64]), object poses and mated_tick ([row][stride]), a policy's act / out
//       ([n_out][stride]) and per-robot points ([walk wave][P][3][64]): one coalesced line per word across the lanes;
//   row-major sources -- u [B][n], the targets [B][ndev][7] (tgt_tile_load: read only, never stored), the feed's wrench [B][ndev][6], all in
//       the record type -- as coalesced tiles through LDS, then read per lane in ascending order and widened exactly;
//   a source that no term names is neither loaded nor given LDS (RewardArgs::need).
// Per-robot state is SoA [field][stride]; the ring of the last ended episodes' (ret, gret) is [IRLOSC_MAX_EPISODE_RECORDS][2][stride] and
// is written by the episode kernel (osc_episode.hpp), beside its own ring.
//
// The arithmetic (include/irlosc.h: "a reward per tick") is float64 whatever the record type, every product, sum, difference and square
// root rounded on its own and in the order written: irl_control_amd/reward.py::reward_tick repeats the bits.  A non-finite reward is
// stored as computed and sets no flag.
//
// init = 1 (irlosc_set_reward): every covered robot's state fresh (reward_fresh); nothing else is read.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/irlosc.h"
#include "osc_common.hpp"

namespace irlosc {

// The reward's per-robot state: r (the last tick's reward), ret and gret (the running episode's plain and discounted sums), disc (gamma
// to the power of the ticks accumulated), steps (those ticks), hold (consecutive ticks the goal's comparison has held), goal_step (steps
// when hold first reached goal_hold; -1: not yet); ring: (ret, gret) of the last ended episodes, entry count mod records
struct RewardState { double* r; double* ret; double* gret; double* disc; int32_t* steps; int32_t* hold; int32_t* goal_step; double* ring; };
constexpr int REWARD_D_ROWS = 4 + 2 * IRLOSC_MAX_EPISODE_RECORDS;      // r, ret, gret, disc, then the ring
constexpr int REWARD_I_ROWS = 3;
// One robot's fresh state (so: its column): what the init launch of irlosc_set_reward leaves -- the setter's fills ARE this function --
// and what a reset of episodes writes.  The ring stays: it belongs to the episodes' count.
__device__ __forceinline__ void reward_fresh(RewardState st, size_t so) {
    st.r[so] = 0.0; st.ret[so] = 0.0; st.gret[so] = 0.0; st.disc[so] = 1.0;
    st.steps[so] = 0; st.hold[so] = 0; st.goal_step[so] = -1;
}

enum : uint32_t { REWARD_NEED_TGT = 1u, REWARD_NEED_U = 2u, REWARD_NEED_WRENCH = 4u };      // the row-major sources a term list names

struct RewardArgs {
    RewardState st;
    const double* xside;           // the tick's exchange block [walk wave][n_entries][64]
    const void* tgt;               // [B][ndev][7] the slot's targets, record type
    const void* u;                 // [B][n] the tick's torques, record type
    const void* wrench;            // [B][ndev][6] the feed's wrench of the tick, record type
    const double* obj_pose;        // [IRLOSC_MAX_OBJECTS 7][stride]
    const int32_t* mated_tick;     // [IRLOSC_MAX_MATES][stride]
    const float* act;              // [n_out][stride]: a Gaussian head's act, else the policy's out
    const double* points;          // per_robot: [walk wave][P][3][64], else [P][3] for the fleet
    double weight[IRLOSC_MAX_REWARD_TERMS];
    double gamma, goal_value;
    int8_t kind[IRLOSC_MAX_REWARD_TERMS], a_kind[IRLOSC_MAX_REWARD_TERMS], a_index[IRLOSC_MAX_REWARD_TERMS], b_kind[IRLOSC_MAX_REWARD_TERMS],
        b_index[IRLOSC_MAX_REWARD_TERMS];
    int32_t ee0[IRLOSC_MAX_DEV];   // exchange entry of each device's EE pose (x y z qw qx qy qz follow each other)
    int32_t n_terms, P, goal_term, goal_cmp, goal_hold;
    uint32_t need;
    int32_t B, n, ndev, n_out, n_entries, stride, per_robot, init;
};

// LDS of a launch: the tiles of the row-major sources the list names, in the order targets, u, wrench (each a 16-byte multiple)
template <typename T>
__host__ __device__ inline size_t reward_tile_bytes(int words) { return ((size_t)64 * words * sizeof(T) + 15) & ~(size_t)15; }
template <typename T>
inline size_t reward_lds_bytes(const RewardArgs& a) {
    return ((a.need & REWARD_NEED_TGT) ? reward_tile_bytes<T>(a.ndev * 7) : 0) + ((a.need & REWARD_NEED_U) ? reward_tile_bytes<T>(a.n) : 0) +
           ((a.need & REWARD_NEED_WRENCH) ? reward_tile_bytes<T>(a.ndev * 6) : 0);
}

template <typename T>
__global__ __launch_bounds__(64) void osc_reward_kernel(const RewardArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
    const int lane = threadIdx.x;
    const int b0 = (int)blockIdx.x * 64;
    const int nvalid = min(64, a.B - b0);           // robots of this wave
    const bool valid = lane < nvalid;
    const size_t so = (size_t)b0 + lane;
    if (a.init) {                                   // (uniform over the launch)
        if (valid) reward_fresh(a.st, so);
        return;
    }
    // ---- the row-major sources the list names, as tiles (the barriers are uniform: `need` is the launch's) ----
    const int trow = a.ndev * 7, wrow = a.ndev * 6;
    unsigned char* sp = s_raw;
    const T* s_t = (const T*)sp;
    if (a.need & REWARD_NEED_TGT) { tgt_tile_load((T*)sp, (const T*)a.tgt + (size_t)b0 * trow, nvalid, trow); sp += reward_tile_bytes<T>(trow); }
    const T* s_u = (const T*)sp;
    if (a.need & REWARD_NEED_U) { tgt_tile_load((T*)sp, (const T*)a.u + (size_t)b0 * a.n, nvalid, a.n); sp += reward_tile_bytes<T>(a.n); }
    const T* s_w = (const T*)sp;
    if (a.need & REWARD_NEED_WRENCH) tgt_tile_load((T*)sp, (const T*)a.wrench + (size_t)b0 * wrow, nvalid, wrow);
    if (!valid) return;                             // (no barrier below; idle lanes of a ragged last wave neither load nor store)

    const double* __restrict__ xs = a.xside + (size_t)blockIdx.x * a.n_entries * 64 + lane;
    const double* __restrict__ pts = a.per_robot ? a.points + (size_t)blockIdx.x * a.P * 3 * 64 + lane : a.points;
    const int ps = a.per_robot ? 64 : 1;            // words between two entries of the robot's points (the fleet's: every lane reads the same word)
    // word c (0..2: position, 3..6: quaternion w x y z) of point (kind, index): the kind is uniform, so one of the four loads is issued
    auto word = [&](int kind, int index, int c) __attribute__((always_inline)) -> double {
        if (kind == IRLOSC_REWARD_EE) return xs[(size_t)(a.ee0[index] + c) * 64];
        if (kind == IRLOSC_REWARD_TARGET) return (double)s_t[lane * trow + index * 7 + c];
        if (kind == IRLOSC_REWARD_OBJECT) return a.obj_pose[(size_t)(index * 7 + c) * a.stride + so];
        return pts[(size_t)(index * 3 + c) * ps];       // FIXED (no orientation: c < 3)
    };
    // sum of three squares, as DIST_SQ sums them
    auto sq3 = [](double x, double y, double z) __attribute__((always_inline)) { return __dadd_rn(__dadd_rn(__dmul_rn(x, x), __dmul_rn(y, y)), __dmul_rn(z, z)); };

    double r = 0.0, vg = 0.0;                       // the tick's reward; the goal term's value
    for (int i = 0; i < a.n_terms; ++i) {
        const int kind = a.kind[i], ak = a.a_kind[i], ai = a.a_index[i], bk = a.b_kind[i], bi = a.b_index[i];
        double v;
        if (kind <= IRLOSC_REWARD_ORI) {            // the terms over two points: the position words 0..2, or (ORI) the quaternion words 3..6
            const bool ori = kind == IRLOSC_REWARD_ORI;
            const int c0 = ori ? 3 : 0;
            double x[4], y[4];                      // (compile-time indices: registers; the loads of a term are in flight together)
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                x[c] = c < 3 || ori ? word(ak, ai, c0 + c) : 0.0;
                y[c] = c < 3 || ori ? word(bk, bi, c0 + c) : 0.0;
            }
            if (ori) {
                double d = __dmul_rn(x[0], y[0]);
#pragma unroll
                for (int c = 1; c < 4; ++c) d = __dadd_rn(d, __dmul_rn(x[c], y[c]));
                v = __dsub_rn(1.0, fabs(d));
            } else {
                v = sq3(__dsub_rn(x[0], y[0]), __dsub_rn(x[1], y[1]), __dsub_rn(x[2], y[2]));
                if (kind == IRLOSC_REWARD_DIST) v = __dsqrt_rn(v);
            }
        } else if (kind == IRLOSC_REWARD_ACT_SQ) {
            float x[7];                             // (at most seven outputs, compile-time indices: the loads are in flight together)
#pragma unroll
            for (int c = 0; c < 7; ++c) x[c] = c < a.n_out ? a.act[(size_t)c * a.stride + so] : 0.0f;
            v = 0.0;
#pragma unroll
            for (int c = 0; c < 7; ++c)
                if (c < a.n_out) v = __dadd_rn(v, __dmul_rn((double)x[c], (double)x[c]));
        } else if (kind == IRLOSC_REWARD_U_SQ) {
            v = 0.0;
#pragma unroll 8
            for (int j = 0; j < a.n; ++j) {
                const double x = (double)s_u[lane * a.n + j];
                v = __dadd_rn(v, __dmul_rn(x, x));
            }
        } else if (kind == IRLOSC_REWARD_FORCE) {
            const T* __restrict__ w = s_w + lane * wrow + ai * 6;
            v = __dsqrt_rn(sq3((double)w[0], (double)w[1], (double)w[2]));
        } else if (kind == IRLOSC_REWARD_MATED) {
            v = a.mated_tick[(size_t)ai * a.stride + so] >= 0 ? 1.0 : 0.0;
        } else {
            v = 1.0;                                // ONE
        }
        r = __dadd_rn(r, __dmul_rn(a.weight[i], v));
        if (i == a.goal_term) vg = v;
    }
    const int steps = a.st.steps[so] + 1;
    const double disc = a.st.disc[so];
    a.st.r[so] = r;
    a.st.steps[so] = steps;
    a.st.ret[so] = __dadd_rn(a.st.ret[so], r);
    a.st.gret[so] = __dadd_rn(a.st.gret[so], __dmul_rn(disc, r));
    a.st.disc[so] = __dmul_rn(disc, a.gamma);
    if (a.goal_term >= 0) {                         // (uniform)
        const bool met = a.goal_cmp ? vg >= a.goal_value : vg <= a.goal_value;      // (a NaN compares false)
        const int hold = met ? a.st.hold[so] + 1 : 0;
        a.st.hold[so] = hold;
        if (hold >= a.goal_hold && a.st.goal_step[so] < 0) a.st.goal_step[so] = steps;
    }
}

}  // namespace irlosc
