// The EPISODES of a rollout (irlosc_set_episodes): per tick and robot the judgement whether its running episode has ended -- its list or
// its non-looping paths are through (FINISHED), or it has been run max_ticks ticks (TIMEOUT) -- and, where it has, the record of the
// episode and the robot's RESET: everything the setters' init launches would leave, so that the robot's next tick is the first tick of a
// fresh rollout while its neighbours go on.  It runs last in a tick, behind the plant: the plant wrote the coordinates a reset replaces,
// the cycler (PATHS) and the action kernel (LIST) have judged the tick, walls and joint rows have written their state.
//
// One lane per robot, one block per walk wave (its 64 robots), like the other program kernels.  What is in force travels as uniform
// launch arguments.  Per-robot state is SoA [field][stride]; the ring of the last `records` ended episodes is [records][4][stride].
//   a QUIET tick (no lane of the wave ends an episode) loads count, age and, by kind, finished_tick or the listed devices' index, and
//     stores age (and start_tick on the first tick that runs an episode); no tile store, no coordinate store;
//   a lane whose episode ENDS writes its record and count, and unless it parks (max_episodes reached) resets: coordinates from start
//     state count mod S (qt in the walk's layout, row-major qpos and qvel), its target row from the snapshot through the wave's target
//     tile (osc_common.hpp: its contract; PATHS: waypoint 0 of every listed device on top), word 9 of the active device's gain record taken
//     again from the context's gains and, with pose variants, the robot's lines of the list's pose table rewritten with variant count mod V,
//     and the FRESH STATE OF EVERY PART IN FORCE -- list, paths of the listed devices, a policy's plate (on the robot's origin), out and grip,
//     walls, action objects (on their start poses count mod OV), their loads, joint rows -- each by the fresh function of the part's own header,
//     which owns the state and its fresh values.  On a slot with mates the record's outcome carries IRLOSC_EPISODE_INSERTED when all of them are mated;
//   with a REWARD in force (osc_reward.hpp; a.reward, uniform like a.walls) a lane whose episode ends writes (ret, gret) into the reward's own
//     ring, entry count mod records beside its record, a reset makes the reward state fresh, and where the reward has a GOAL (a.goal) an
//     episode is also finished by goal_step >= 0 -- whatever the program -- and one that ends with it carries IRLOSC_EPISODE_GOAL;
//   idle lanes of a ragged last wave neither load nor store.
// Every wave stores the number of its robots that are not parked into running[walk wave] (a plain store by lane 0): the early exit's input.
//
// init = 1 (irlosc_set_episodes): count 0, age 0, start_tick -1, start state 0 into the coordinates, variant 0 into the list's table, and
// the snapshot of the targets is taken; nothing else is touched.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/irlosc.h"
#include "osc_common.hpp"
#include "osc_action.hpp"
#include "osc_waypoint.hpp"
#include "osc_policy.hpp"
#include "osc_wall.hpp"
#include "osc_joint.hpp"
#include "osc_object.hpp"
#include "osc_object_load.hpp"
#include "osc_reward.hpp"

namespace irlosc {

enum : int32_t { EP_NONE = 0, EP_PATHS = 1, EP_LIST = 2, EP_POLICY = 3 };      // the program in force on the tick (Program::Kind of irlosc.hip, STREAM refused)

struct EpisodeArgs {
    int32_t* count;           // [stride] each
    int32_t* age;
    int32_t* start_tick;
    int32_t* ring;            // [records][4][stride]: start_tick, length, outcome, start | variant << 16
    int32_t* running;         // [walk waves]
    double* qt;               // [walk wave][2 NJ][64]
    double* qpos;             // [B][NJ] row-major
    double* qvel;
    const double* starts;     // starts_per_robot: [walk wave][S][2 NJ][64], else [S][2 NJ]; entry 2 j = q_j, 2 j + 1 = qd_j
    void* tgt;                // [B][ndev][7] targets of the slot, record type
    void* snap;               // ... their snapshot
    ListState ls;             // LIST (osc_action.hpp)
    double* al_table;         // list_per_robot: [walk wave][A][7][64], else [A][7]
    const double* variants;   // [V] tables of that layout, vstride doubles apart
    void* al_gains;           // [B][ndev][IRLOSC_GAIN_WORDS] the slot's gain copy, record type
    const void* gains;        // the context's gains, record type: [1 | max_batch][ndev][IRLOSC_GAIN_WORDS]
    PathState wp;             // PATHS (osc_waypoint.hpp)
    const double* wp_table;   // wp_per_robot: [walk wave][ndev][wmax][3][64], else [ndev][wmax][3]
    // POLICY (osc_policy.hpp): never finished by itself -- its episodes end by max_ticks, or on a reward's goal; a reset puts the plate back to the robot's origin
    PlateState pl;
    const double* pl_origin;  // per robot: [walk wave][6][64]; nullptr: pl_origin0 for the fleet
    double pl_origin0[6];
    PolicyState po;
    int32_t pl_n_out, pl_pad;
    WallState wl;             // walls (osc_wall.hpp)
    JointState jt;            // joint rows (osc_joint.hpp)
    ObjectState ob;           // action objects (osc_object.hpp) ...
    const double* ob_pose0;   // ... their start poses [OV][walk wave][nobj 7][64], ob_vstride doubles apart
    int64_t ob_vstride;
    int32_t objects, nobj, ng, nm, OV;
    LoadState ld;             // the carried objects' weight (osc_object_load.hpp)
    int32_t loads, ld_pad;
    RewardState rw;           // the reward (osc_reward.hpp): reward: one is in force; goal: it has a goal, which ends an episode like a finished program
    int32_t reward, goal;
    int64_t vstride;
    int32_t wp_count[IRLOSC_MAX_DEV];
    uint8_t wp_loop[IRLOSC_MAX_DEV];
    int32_t B, ndev, stride, kind, walls, joints, R, A, S, V, wmax;
    int32_t starts_per_robot, list_per_robot, wp_per_robot, gains_per_robot, active;
    int32_t max_ticks, end_on_finish, max_episodes, records, tick, init;
};

template <class TOPO, typename T>
__global__ __launch_bounds__(64) void osc_episode_kernel(const EpisodeArgs a) {
    constexpr int NJ = TOPO::NJ;
    __shared__ T s_t[64 * IRLOSC_MAX_DEV * 7];      // the wave's target tile
    const int lane = threadIdx.x;
    const int b0 = (int)blockIdx.x * 64;
    const int nvalid = min(64, a.B - b0);           // robots of this wave
    const bool valid = lane < nvalid;
    const size_t so = (size_t)b0 + lane;
    const int row = a.ndev * 7;
    T* __restrict__ tg = (T*)a.tgt + (size_t)b0 * row;
    T* __restrict__ sn = (T*)a.snap + (size_t)b0 * row;
    int cnt = 0;
    bool ends = false, reset = false;
    if (a.init) {                                   // (uniform over the launch)
        tgt_tile_load(s_t, tg, nvalid, row);
        for (int t = 0; t < row; ++t) {
            const int i = t * 64 + lane;
            if (i < nvalid * row) sn[i] = s_t[i];
        }
        if (valid) { a.count[so] = 0; a.age[so] = 0; a.start_tick[so] = -1; }
    } else if (valid) {                             // idle lanes load nothing
        cnt = a.count[so];
        const int age0 = a.age[so];
        const bool parked = a.max_episodes > 0 && cnt >= a.max_episodes;
        bool fin = false;
        if (a.end_on_finish && a.kind == EP_LIST) fin = a.ls.finished_tick[so] >= 0;
        if (a.end_on_finish && a.kind == EP_PATHS) {
            bool all = true, some = false;
            for (int d = 0; d < a.ndev; ++d)
                if (a.wp_count[d] > 0 && !a.wp_loop[d]) {
                    some = true;
                    all = all & (a.wp.index[(size_t)d * a.stride + so] == a.wp_count[d]);
                }
            fin = some & all;
        }
        const bool goal = a.goal && a.rw.goal_step[so] >= 0;      // (a.goal: uniform; this tick's reward kernel has judged the tick)
        if (a.end_on_finish) fin = fin | goal;
        const int age = parked ? age0 : age0 + 1;   // a parked robot is never judged again
        const bool tmo = a.max_ticks > 0 && age == a.max_ticks;
        ends = !parked && (fin | tmo);
        const bool first = !parked && age0 == 0;    // the first tick that runs this episode
        if (first) a.start_tick[so] = a.tick;
        if (ends) {
            int32_t* __restrict__ r = a.ring + ((size_t)(cnt % a.records) * 4) * a.stride + so;
            r[0] = first ? a.tick : a.start_tick[so];
            r[(size_t)a.stride] = age;
            int outcome = fin ? IRLOSC_EPISODE_FINISHED : IRLOSC_EPISODE_TIMEOUT;
            if (a.nm > 0) {                         // a slot with mates: every one of them mated by this tick's object kernel
                bool all = true;
                for (int m = 0; m < a.nm; ++m) all = all & (a.ob.mated_tick[(size_t)m * a.stride + so] >= 0);
                if (all) outcome |= IRLOSC_EPISODE_INSERTED;
            }
            if (goal) outcome |= IRLOSC_EPISODE_GOAL;
            r[2 * (size_t)a.stride] = outcome;
            if (a.reward) {                         // (ret, gret) of the episode, beside its record
                double* __restrict__ rr = a.rw.ring + ((size_t)(cnt % a.records) * 2) * a.stride + so;
                rr[0] = a.rw.ret[so];
                rr[(size_t)a.stride] = a.rw.gret[so];
            }
            r[3 * (size_t)a.stride] = (cnt % a.S) | ((a.V > 0 ? cnt % a.V : 0) << 16);
            cnt += 1;
            a.count[so] = cnt;
            reset = a.max_episodes == 0 || cnt < a.max_episodes;
            if (reset) a.start_tick[so] = -1;
        }
        if (!parked) a.age[so] = reset ? 0 : age;
    }
    // the fleet's state for the early exit
    {
        const bool still = valid && !(a.max_episodes > 0 && cnt >= a.max_episodes);
        const unsigned long long m = __ballot(still);
        if (lane == 0) a.running[blockIdx.x] = __popcll(m);
    }
    const bool fresh = reset || (a.init && valid);  // the lanes that get a start state (and a variant)
    if (fresh) {
        // ---- coordinates: start state count mod S, in the walk's layout and row-major ----
        const int s = cnt % a.S;
        const double* __restrict__ src = a.starts_per_robot ? a.starts + (((size_t)blockIdx.x * a.S + s) * (2 * NJ)) * 64 + lane
                                                            : a.starts + (size_t)s * (2 * NJ);
        const int cs = a.starts_per_robot ? 64 : 1;
        double* __restrict__ qc = a.qt + (size_t)blockIdx.x * (2 * NJ * 64) + lane;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const double q = src[(size_t)(2 * j) * cs], qd = src[(size_t)(2 * j + 1) * cs];
            qc[(2 * j) * 64] = q;
            qc[(2 * j + 1) * 64] = qd;
            a.qpos[so * NJ + j] = q;
            a.qvel[so * NJ + j] = qd;
        }
        // ---- the list's pose table: this robot's lines from variant count mod V ----
        if (a.kind == EP_LIST && a.V > 0) {
            const double* __restrict__ vs = a.variants + (size_t)(cnt % a.V) * a.vstride;
            const int E = a.A * 7;
            const size_t o = a.list_per_robot ? ((size_t)blockIdx.x * E) * 64 + lane : 0;
            const int ls = a.list_per_robot ? 64 : 1;
            for (int e = 0; e < E; ++e) a.al_table[o + (size_t)e * ls] = vs[o + (size_t)e * ls];
        }
    }
    if (reset) {                                    // THE branch around the reset body (state; the targets follow through the tile)
        if (a.kind == EP_LIST) {                    // ... and word 9 of the active device's gain record taken again
            list_fresh(a.ls, a.stride, so);
            const size_t w9 = (size_t)a.active * IRLOSC_GAIN_WORDS + 9;
            ((T*)a.al_gains)[so * a.ndev * IRLOSC_GAIN_WORDS + w9] = ((const T*)a.gains)[(a.gains_per_robot ? so : 0) * a.ndev * IRLOSC_GAIN_WORDS + w9];
        }
        for (int d = 0; a.kind == EP_PATHS && d < a.ndev; ++d) {      // the listed devices
            if (a.wp_count[d] <= 0) continue;
            path_fresh(a.wp, (size_t)d * a.stride + so, a.wp_count[d]);
        }
        if (a.kind == EP_POLICY) {                  // the plate on the robot's origin
            double origin[6];
#pragma unroll
            for (int c = 0; c < 6; ++c) origin[c] = a.pl_origin ? a.pl_origin[((size_t)blockIdx.x * 6 + c) * 64 + lane] : a.pl_origin0[c];
            plate_fresh(a.pl, a.stride, so, origin);
            policy_fresh(a.po, a.pl_n_out, a.stride, so);
        }
        if (a.walls) wall_fresh(a.wl, a.ndev, a.stride, so);
        if (a.objects)                              // on start poses count mod OV
            object_fresh(a.ob, a.ob_pose0 + (size_t)(cnt % a.OV) * a.ob_vstride + (size_t)blockIdx.x * a.nobj * 7 * 64 + lane, a.nobj, a.ng, a.nm, (size_t)a.stride, so);
        if (a.loads) load_fresh(a.ld, a.ng, (size_t)a.stride, so);
        if (a.joints) joint_fresh<NJ>(a.jt, a.R, a.stride, so);
        if (a.reward) reward_fresh(a.rw, so);
    }
    // ---- targets: the whole row back from the snapshot, through the wave's tile; only a wave in which a lane reset touches it ----
    if (!a.init && __any(reset)) {                  // (one wave per block: uniform over the block)
        tgt_tile_load(s_t, tg, nvalid, row);
        if (reset) {
            T* t = s_t + lane * row;
            const T* __restrict__ p = sn + lane * row;
            for (int c = 0; c < row; ++c) t[c] = p[c];
            if (a.kind == EP_PATHS) {               // waypoint 0 of every listed device, as the cycler's init
                for (int d = 0; d < a.ndev; ++d) {
                    if (a.wp_count[d] <= 0) continue;
                    const size_t e = ((size_t)d * a.wmax) * 3;
                    const double* __restrict__ w = a.wp_per_robot ? a.wp_table + ((size_t)blockIdx.x * a.ndev * a.wmax * 3 + e) * 64 + lane : a.wp_table + e;
                    const int ws = a.wp_per_robot ? 64 : 1;
#pragma unroll
                    for (int c = 0; c < 3; ++c) t[d * 7 + c] = (T)w[c * ws];
                }
            }
        }
        tgt_tile_store(tg, s_t, nvalid, row, reset);
    }
}

}  // namespace irlosc
