// libirlosc.so — C ABI (include/irlosc.h) over the gfx950 OSC kernels.  No CPU fallback: every
// compute entry point needs a HIP device and reports IRLOSC_ERR_HIP otherwise.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>      // types only: the library is dlopen()ed on first use
#include <dlfcn.h>

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <algorithm>
#include <array>
#include <cmath>
#include <type_traits>
#include <vector>

#include "../../include/irlosc.h"
#include "osc_common.hpp"
#include "osc_generic.hpp"
#include "osc_assemble.hpp"
#include "osc_row16.hpp"
#include "osc_frontend.hpp"
#include "osc_lane_types.hpp"
#include "osc_ft.hpp"
#include "osc_pack.hpp"
#include "osc_plant.hpp"
#include "osc_waypoint.hpp"
#include "osc_action.hpp"
#include "osc_teleop.hpp"
#include "osc_policy.hpp"
#include "osc_object.hpp"
#include "osc_push.hpp"
#include "osc_wall.hpp"
#include "osc_object_load.hpp"
#include "osc_joint.hpp"
#include "osc_reward.hpp"
#include "osc_log.hpp"
#include "osc_episode.hpp"
#include "launchers.hpp"
#include "dev_mem.hpp"

using namespace irlosc;
static_assert(FE_TRAIN == R16_TRAIN, "the walk and the OSC kernel chain the same number of steps per launch");
static_assert(FT_TRAIN == R16_TRAIN, "the sensor-feed wrench kernel covers a whole train");

static thread_local std::string g_create_error;

// The program that writes a slot's targets inside a rollout, if any: waypoint paths (irlosc_set_waypoints, osc_waypoint.hpp), the
// WP / GRIP action list (irlosc_set_action_list, osc_action.hpp), a teleoperation stream (irlosc_set_teleop_stream, osc_teleop.hpp) or a
// policy (irlosc_set_policy, osc_policy.hpp).  One entry point writes the targets at a time, so a slot has one program at most -- `kind`
// says which: paths, a list, a stream and a policy exclude each other.  Written by the transitions below and by nothing else.
struct Program {
    enum Kind { NONE, PATHS, LIST, STREAM, POLICY };
    Kind kind = NONE;          // (NONE: a rollout tick launches none of the kernels and reads the context's gains)
    int robots = 0, tick = 0;  // robots the program covers; rollout ticks since it came in force
    irlosc_waypoints wp{};     // the description in force: of paths; of a list; of a stream
    irlosc_action_list al{};
    irlosc_teleop_stream ts{};  // (a policy: its rig in a stream's form, which is what the shared body reads)
    irlosc_policy po{};
    std::vector<double> ts_shared;      // a shared stream's readings [T][6]: they travel as kernel arguments, tick by tick
    int refs = 0;              // 1: the list aims at the slot's action objects as `rf` says (irlosc_set_action_refs)
    irlosc_action_refs rf{};
    int motion = 0;            // 1: the list's WPs travel and scatter as `am` says (irlosc_set_action_motion): its ticks launch the MOTION kernel
    irlosc_action_motion am{};
    DevBuf<int32_t> am_i;      // the motion's per-robot state, allocated by its first use for max_batch robots: step, draws (uint32) ...
    DevBuf<double> am_d;       // ... origin[7], goal[7]
    int32_t* m_step(size_t) const { return am_i; }  uint32_t* m_draws(size_t Bm) const { return (uint32_t*)(am_i + Bm); }
    double* m_origin(size_t) const { return am_d; }  double* m_goal(size_t Bm) const { return am_d + 7 * Bm; }
    static size_t am_i_words(size_t Bm) { return 2 * Bm; }  static size_t am_d_words(size_t Bm) { return 14 * Bm; }
    // Device buffers, allocated by the first use and kept across programs: per-robot state SoA over max_batch robots (wp_i, al_i, al_d), the
    // table (walk_table), and a list's own gains [robots][ndev][12] and null_kv [robots] in the context's dtype (its rollout reads these per instance)
    // A stream: the pose SoA [6][max_batch] (ts_pose), per-robot readings (ts_table) and per-robot origins (ts_origin), both walk_table.
    DevBuf<int32_t> wp_i, al_i;
    DevBuf<double> wp_table, al_d, al_table, ts_pose, ts_table, ts_origin;
    DevBuf<void> al_gains, al_nullkv;
    // A policy: the network as the kernel walks it (po_net) over the packed weights (po_w); per-robot state out [n_out][max_batch] (po_out) and grip
    // [max_batch] (po_grip), the kept observation [robots][n_in] (po_obs); the pose and per-robot origins are the stream's ts_pose and ts_origin;
    // a fleet-wide origin (po_origin0) and the objects the observation was sized for (po_nobj; -1: it does not look at them) stay on the host
    PolicyNet po_net{};
    double po_origin0[6] = {};
    int po_nobj = -1;
    DevBuf<float> po_w, po_out, po_obs;
    DevBuf<double> po_grip;
    // The Gaussian head of the policy in force (irlosc_set_policy_noise): the description (pn), C of logp (pn_const), and its per-robot
    // state, allocated by the first use for max_batch robots: act [n_out][max_batch], logp [max_batch], draws [max_batch]
    int noise = 0;             // 1: the policy's ticks launch the NOISE form of its kernel
    irlosc_policy_noise pn{};
    double pn_const = 0.0;
    DevBuf<float> pn_act;
    DevBuf<double> pn_logp;
    DevBuf<uint32_t> pn_draws;
    // THE LAYOUT of the state -- the kernels' arguments, the setters' sizes and the downloads all ask here: wp_i in planes of `plane` =
    // ndev x max_batch words; al_i and al_d in rows of Bm = max_batch words (start_xyz: three rows); and their sizes
    int32_t* index(size_t) const { return wp_i; }  int32_t* arrivals(size_t plane) const { return wp_i + plane; }  int32_t* last_tick(size_t plane) const { return wp_i + 2 * plane; }
    int32_t* action(size_t) const { return al_i; }  int32_t* entered(size_t Bm) const { return al_i + Bm; }  int32_t* grip_left(size_t Bm) const { return al_i + 2 * Bm; }
    int32_t* finished_tick(size_t Bm) const { return al_i + 3 * Bm; }
    double* err(size_t) const { return al_d; }  double* max_vel0(size_t Bm) const { return al_d + Bm; }  double* gripper_force(size_t Bm) const { return al_d + 2 * Bm; }
    double* start_xyz(size_t Bm) const { return al_d + 3 * Bm; }
    double* pose(size_t) const { return ts_pose; }      // (x y z roll pitch yaw: six rows of Bm words)
    static size_t wp_words(size_t plane) { return 3 * plane; }  static size_t al_i_words(size_t Bm) { return 4 * Bm; }  static size_t al_d_words(size_t Bm) { return 6 * Bm; }
    static size_t ts_words(size_t Bm) { return 6 * Bm; }
    // ... and each kind's state as its kernels and a reset of episodes take it (the structs of osc_action.hpp, osc_waypoint.hpp, osc_teleop.hpp, osc_policy.hpp)
    ListState list_state(size_t Bm) const { return {action(Bm), entered(Bm), grip_left(Bm), finished_tick(Bm), err(Bm), max_vel0(Bm), gripper_force(Bm), start_xyz(Bm)}; }
    MotionState motion_state(size_t Bm) const { return {m_step(Bm), m_draws(Bm), m_origin(Bm), m_goal(Bm)}; }  PlateState plate_state(size_t Bm) const { return {pose(Bm)}; }
    PathState path_state(size_t plane) const { return {index(plane), (uint32_t*)arrivals(plane), last_tick(plane)}; }  PolicyState policy_state() const { return {po_out, po_grip, noise ? pn_act.get() : nullptr, noise ? pn_logp.get() : nullptr, noise ? pn_draws.get() : nullptr}; }

    // Paths of B robots are in force, their state reset by the cycler's init launch (which also wrote waypoint 0 into the targets).
    void paths(int B, const irlosc_waypoints& d) { kind = PATHS; robots = B; tick = 0; wp = d; }
    // A list of B robots is in force, its state reset by the kernel's init launch and its gain copy made: it writes the targets from here on.
    void list(int B, const irlosc_action_list& d) { kind = LIST; robots = B; tick = 0; al = d; refs = 0; motion = 0; }
    // The list in force has a motion, its state on the device / jumps from pose to pose again (its motion was cleared)
    void moves(const irlosc_action_motion& m) { motion = 1; am = m; }
    void still() { motion = 0; }
    // The list in force aims at the slot's objects / at its own table alone again (its refs were cleared, or the objects they name changed)
    void aims(const irlosc_action_refs& r) { refs = 1; rf = r; }
    void aimless() { refs = 0; }
    // A stream over B robots is in force, their poses at the origins by the kernel's init launch (which wrote no target: the first tick
    // does); `shared`: the readings of a stream for the whole fleet.
    void stream(int B, const irlosc_teleop_stream& d, std::vector<double>&& shared) { kind = STREAM; robots = B; tick = 0; ts = d; ts_shared = std::move(shared); }
    // A policy over B robots is in force, their poses at the origins by the stream kernel's init launch, out and grip zero (no target written: the first tick does)
    void policy(int B, const irlosc_policy& d, const irlosc_teleop_stream& rig, const PolicyNet& net, int nobj, const double* origin0) {
        kind = POLICY; robots = B; tick = 0; po = d; ts = rig; po_net = net; po_nobj = nobj; noise = 0;      // (a new policy has no head)
        for (int i = 0; i < 6; ++i) po_origin0[i] = origin0[i];
    }
    // The reading a stream takes on the tick to come: tick mod T of one that loops, none (-1) once one that does not has ended
    int reading() const { return kind != STREAM ? -1 : ts.loop ? tick % ts.ticks : tick < ts.ticks ? tick : -1; }
    // The program ends: irlosc_set_targets wrote the targets, another program takes them over, the model changed, or its buffers failed.
    void end() { kind = NONE; robots = 0; tick = 0; refs = 0; motion = 0; noise = 0; }
    // The policy in force has a Gaussian head, its state on the device / is deterministic again (its head was cleared)
    void samples(const irlosc_policy_noise& d, double logp_const) { noise = 1; pn = d; pn_const = logp_const; }
    void exact() { noise = 0; }
    // The program ends if it is of this kind (its own setter cleared it; a list: the gains its copy was made from were replaced): one of the other kind stays whole
    void end(Kind k) { if (kind == k) end(); }
    // A tick of a rollout ran the program's kernel.  (Marked once the whole tick is enqueued: if a launch behind the kernel fails, the
    // device state is one tick ahead of `tick` -- on a context whose stream has already failed, where the rollout's result is void anyway.)
    void ticked() { ++tick; }
};

// What acts on the plant inside a slot's rollouts: external pushes, compliant walls, joint rows (below).  None of them writes targets, so
// none is a Program: they live next to one and next to each other.  Each is written by its set(), by end() and ticked(), and by nothing else.
struct PlantForce {
    int robots = 0, tick = 0;  // robots it covers (0: none); rollout ticks since it came in force
    DevBuf<double> table;      // its table (walk_table), allocated by the first use, kept across settings and grown on demand
    // It ends: its setter cleared it, the model changed (hinge indices and the block's entry layout are the model's), or its buffers failed.
    void end() { robots = 0; tick = 0; }
    // A tick of a rollout ran (with or without a launch of its own: the pushes' windows are judged on the host).
    void ticked() { if (robots) ++tick; }
protected:
    // It is in force for B robots, its table and (where it has some) its reset state on the device.
    void in_force(int B) { robots = B; tick = 0; }
};

// The external pushes (irlosc_set_pushes, osc_push.hpp): wrenches on EE bodies during windows of ticks, applied to the plant and / or
// taken off the sensor feed's wrench a tick later.
struct Pushes : PlantForce {
    irlosc_pushes d{};         // the description in force
    void set(int B, const irlosc_pushes& desc) { in_force(B); d = desc; }
    // The pushes whose window holds tick t and that act on the plant / are read by the sensors: bit p
    uint32_t active(int t, const uint8_t* which) const {
        uint32_t m = 0;
        for (int p = 0; robots && t >= 0 && p < d.n_pushes; ++p)
            if (which[p] && d.tick0[p] <= t && t < d.tick1[p]) m |= 1u << p;
        return m;
    }
    uint32_t applied() const { return active(tick, d.apply); }        // on this tick
    uint32_t sensed() const { return active(tick - 1, d.sense); }     // on this tick: what the step of the tick before felt
};

// The compliant walls (irlosc_set_walls, osc_wall.hpp): penalty half-spaces on EE bodies, their force computed on the device per robot
// and tick, applied to the plant and taken off the sensor feed's wrench a tick later.
struct Walls : PlantForce {
    irlosc_walls d{};          // the description in force
    DevBuf<double> st_d;       // per-robot state, allocated by the first use for max_batch robots: force xyz, max_depth
    DevBuf<int32_t> st_i;      // ... contact_ticks, first_tick
    // THE LAYOUT of the state: st_d / st_i in planes of `plane` = ndev x max_batch words (force: a plane per axis), and their sizes
    double* force(size_t plane, size_t axis = 0) const { return st_d + axis * plane; }  double* max_depth(size_t plane) const { return st_d + 3 * plane; }
    int32_t* contact_ticks(size_t) const { return st_i; }  int32_t* first_tick(size_t plane) const { return st_i + plane; }
    static size_t d_words(size_t plane) { return 4 * plane; }  static size_t i_words(size_t plane) { return 2 * plane; }
    WallState state(size_t plane) const { return {force(plane), max_depth(plane), contact_ticks(plane), first_tick(plane)}; }
    void set(int B, const irlosc_walls& desc) { in_force(B); d = desc; }
    // The devices that have a wall: bit d
    uint32_t devices() const {
        uint32_t m = 0;
        for (int w = 0; robots && w < d.n_walls; ++w) m |= 1u << d.dev[w];
        return m;
    }
};

// The joint rows (irlosc_set_joints, osc_joint.hpp): range stops, finger couplings and gripper drives, one torque per hinge computed
// on the device per robot and tick and taken off the bias in front of the plant.
struct Joints : PlantForce {
    irlosc_joint_rows d{};     // the description in force
    DevBuf<double> st_d;       // per-robot state, grown on demand: tau[MAX_N] (the kernel writes its tree's NJ hinges), max_violation[R], ctrl[R]
    DevBuf<int32_t> st_i;      // ... active_ticks[R]
    // THE LAYOUT of the state: st_d / st_i in rows of Bm = max_batch words, for R rows, and their sizes
    double* tau(size_t) const { return st_d; }  double* max_violation(size_t Bm) const { return st_d + (size_t)IRLOSC_MAX_N * Bm; }
    double* ctrl(size_t Bm, size_t R) const { return st_d + ((size_t)IRLOSC_MAX_N + R) * Bm; }  int32_t* active_ticks(size_t) const { return st_i; }
    static size_t d_words(size_t Bm, size_t R) { return ((size_t)IRLOSC_MAX_N + 2 * R) * Bm; }  static size_t i_words(size_t Bm, size_t R) { return R * Bm; }
    JointState state(size_t Bm) const { return {tau(Bm), max_violation(Bm), ctrl(Bm, d.n_rows), active_ticks(Bm)}; }      // (of the rows in force)
    void set(int B, const irlosc_joint_rows& desc) { in_force(B); d = desc; }
};

// The action objects (irlosc_set_objects, osc_object.hpp): kinematic bodies a gripper carries.  By themselves they act on nothing -- no force on the
// plant, none in the feed: that is their Loads', below -- but live here with the parts that have a table (the start poses), per-robot state and a tick of their own.
struct Objects : PlantForce {
    irlosc_objects d{};        // the description in force
    size_t vstride = 0;        // doubles between two variants' start poses in `table` ([V][walk wave][nobj 7][64])
    DevBuf<double> st_d;       // per-robot state, allocated by the first use for max_batch robots: pose, rel
    DevBuf<int32_t> st_i;      // ... holder, grasp_tick, release_tick, was_closed, mated_tick
    // THE LAYOUT of the state (osc_object.hpp): rows of Bm = max_batch words
    double* pose(size_t) const { return st_d; }  double* rel(size_t Bm) const { return st_d + (size_t)OBJ_POSE_ROWS * Bm; }
    int32_t* holder(size_t) const { return st_i; }  int32_t* grasp_tick(size_t Bm) const { return st_i + (size_t)IRLOSC_MAX_OBJECTS * Bm; }
    int32_t* release_tick(size_t Bm) const { return st_i + 2 * (size_t)IRLOSC_MAX_OBJECTS * Bm; }
    int32_t* was_closed(size_t Bm) const { return st_i + 3 * (size_t)IRLOSC_MAX_OBJECTS * Bm; }
    int32_t* mated_tick(size_t Bm) const { return st_i + (3 * (size_t)IRLOSC_MAX_OBJECTS + IRLOSC_MAX_GRIPPERS) * Bm; }
    static size_t d_words(size_t Bm) { return (size_t)OBJ_D_ROWS * Bm; }  static size_t i_words(size_t Bm) { return (size_t)OBJ_I_ROWS * Bm; }
    ObjectState state(size_t Bm) const { return {pose(Bm), rel(Bm), holder(Bm), grasp_tick(Bm), release_tick(Bm), was_closed(Bm), mated_tick(Bm)}; }
    void set(int B, const irlosc_objects& desc, size_t vs) { in_force(B); d = desc; vstride = vs; }
    int count() const { return robots ? d.n_objects : 0; }      // objects of the slot (0: it has none)
};

// The carried objects' weight (irlosc_set_object_loads, osc_object_load.hpp): a side description of the slot's objects -- per object a
// mass and a centre of mass, and gravity -- whose wrench on the holder's EE body is computed on the device per robot and tick, applied to
// the plant and taken off the sensor feed's wrench a tick later.  They live and end with the objects they describe.
struct Loads : PlantForce {
    irlosc_object_loads d{};   // the description in force (per_robot: how `table` is laid out -- a lone robot's is the shared form)
    DevBuf<double> st_d;       // per-robot state, allocated by the first use for max_batch robots: load[MAX_GRIPPERS 6]
    DevBuf<int32_t> st_i;      // ... carry_ticks[MAX_GRIPPERS]
    // THE LAYOUT of the state (osc_object_load.hpp): rows of Bm = max_batch words
    double* load(size_t) const { return st_d; }  int32_t* carry_ticks(size_t) const { return st_i; }
    static size_t d_words(size_t Bm) { return (size_t)IRLOSC_MAX_GRIPPERS * 6 * Bm; }  static size_t i_words(size_t Bm) { return (size_t)IRLOSC_MAX_GRIPPERS * Bm; }
    LoadState state(size_t Bm) const { return {load(Bm), carry_ticks(Bm)}; }
    void set(int B, const irlosc_object_loads& desc) { in_force(B); d = desc; }
};

// The reward (irlosc_set_reward, osc_reward.hpp): per robot and tick a list of weighted terms over the tick's state, accumulated per episode,
// with an optional goal.  It writes no targets and acts on nothing; it READS other parts by name, so what it names is checked by its setter
// and again by every rollout call (check_reward_refs).  Written by set() and end(), and by nothing else.
struct Reward {
    irlosc_reward d{};         // the description in force
    int robots = 0;            // robots it covers (0: none)
    int per_robot = 0;         // how `table` is laid out (a lone robot's: the shared form)
    DevBuf<double> table;      // its points (walk_table), grown on demand
    DevBuf<double> st_d;       // per-robot state, allocated by the first use for max_batch robots: r, ret, gret, disc, the ring
    DevBuf<int32_t> st_i;      // ... steps, hold, goal_step
    // Which episodes its ring's entries can stem from: the serial of the episodes in force when it was set (-1: none) and their tick then
    long ep_serial = -1;
    int ep_tick0 = 0;
    // THE LAYOUT of the state (osc_reward.hpp): rows of Bm = max_batch words; the ring [IRLOSC_MAX_EPISODE_RECORDS][2][Bm] behind the doubles
    static size_t d_words(size_t Bm) { return (size_t)REWARD_D_ROWS * Bm; }  static size_t i_words(size_t Bm) { return (size_t)REWARD_I_ROWS * Bm; }
    RewardState state(size_t Bm) const { return {st_d, st_d + Bm, st_d + 2 * Bm, st_d + 3 * Bm, st_i, st_i + Bm, st_i + 2 * Bm, st_d + 4 * Bm}; }
    bool goal() const { return robots && d.goal_term >= 0; }
    void set(int B, const irlosc_reward& desc, int pr, long serial, int tick0) { robots = B; d = desc; per_robot = pr; ep_serial = serial; ep_tick0 = tick0; }
    // It ends: its setter cleared it, the model changed, or its buffers failed.
    void end() { robots = 0; }
};

// The episodes (irlosc_set_episodes, osc_episode.hpp): per robot the judgement whether its running episode has ended, its record and its
// reset on the device, and per wave the robots still running for the early exit.  They write no targets but a reset robot's snapshot row,
// so they are no Program: they live next to one.  Written by laid_out(), set(), end() and ticked(), and by nothing else.
struct Episodes {
    irlosc_episodes d{};       // the description in force
    int robots = 0, tick = 0;  // robots they cover (0: none); rollout ticks since they came in force
    long serial = 0;           // counts the settings that came in force (the reward's ring asks which one wrote an entry)
    int starts_per_robot = 0, list_per_robot = 0;      // the layouts of `starts` and of the list's pose table (a lone robot's: the shared one)
    size_t vstride = 0;        // doubles between two variants' tables
    DevBuf<int32_t> st_i;      // per-robot state, allocated by the first use for max_batch robots: count, age, start_tick, the ring
    DevBuf<int32_t> running;   // [walk waves of max_batch]
    DevBuf<void> snap;         // the targets' snapshot [max_batch][ndev][7], record type
    DevBuf<double> starts, variants;      // the start states and the pose variants (walk_table), grown on demand
    // THE LAYOUT of the state: rows of Bm = max_batch words; the ring [IRLOSC_MAX_EPISODE_RECORDS][4][Bm] behind them
    int32_t* count(size_t) const { return st_i; }  int32_t* age(size_t Bm) const { return st_i + Bm; }  int32_t* start_tick(size_t Bm) const { return st_i + 2 * Bm; }
    int32_t* ring(size_t Bm) const { return st_i + 3 * Bm; }
    static size_t i_words(size_t Bm) { return (3 + 4 * (size_t)IRLOSC_MAX_EPISODE_RECORDS) * Bm; }
    // Episodes of B robots are in force: tables, snapshot and reset state on the device.  (They belong to the program in force with them:
    // every transition that ends or replaces it ends them.)
    void set(int B, const irlosc_episodes& desc) { robots = B; tick = 0; d = desc; ++serial; }
    // The tables of the episodes to come are laid out like this (ahead of the init launch, which reads them; none are in force meanwhile)
    void laid_out(int starts_pr, int list_pr, size_t vs) { starts_per_robot = starts_pr; list_per_robot = list_pr; vstride = vs; }
    // They end: their setter cleared them, the model changed, the targets or the program they were set on changed, or their buffers failed.
    void end() { robots = 0; tick = 0; }
    // A tick of a rollout ran their kernel.
    void ticked() { if (robots) ++tick; }
};

// One slot of a context: the resident inputs of a step, grouped by what they describe.  Records and targets come with the context
// (create_impl); the other buffers are allocated by their first use -- qpos / qvel by the first irlosc_set_model, qt by the first use while
// the fused path is on, sens by the slot's first feed, blk / blk_dq by its first pack.  Counts: 0 = nothing yet, -1 = an
// empty batch.
// The state of the records and of what follows them is written by the transitions below and by nothing else.  INVARIANT: `tree` and
// `packed` -- and so the route irlosc_slot_route reports -- are non-zero only while `records` > 0: every transition that lowers
// `records` clears both, and only accepted() / block_packed() raise them.  (targets / has_tvel, coords and feed count
// independent inputs, each written by its one entry point: irlosc_set_targets, irlosc_upload_q, irlosc_set_sensordata.)
struct Slot {
    // dense records
    DevBuf<void> M, J, dq, bias, ee, wrench;
    int records = 0;           // instances they hold
    int has_wrench = 0;
    int tree = 0;              // 1: verified to carry the zero pattern of the compiled Dual-UR5 tree (probe), or written by the lane front end
    int fused_away = 0;        // 1: invalidated by a fused step from joint coordinates (error text only)
    // their compact block for the resident lane route ([walk wave][n_compact][64 robots], 2.7 KB per robot) and dq in the walk's
    // coordinate layout ([walk wave][2 n][64], entry 2 j + 1 = dq_j)
    DevBuf<double> blk, blk_dq;
    int packed = 0;            // robots packed (0: no valid block -- the slot steps on the row16 kernel)
    // targets
    DevBuf<void> tgt, tvel;
    int targets = 0, has_tvel = 0;
    // joint coordinates; qt: the same in the fused walk's layout [wave][2 n][64 robots] (irlosc_upload_q writes both)
    DevBuf<double> qpos, qvel, qt;
    int coords = 0;
    // F/T sensor feed of the steps from joint coordinates: the sensordata (the wrench computed from it is a buffer of the step's
    // bank, Bank::ftw)
    DevBuf<double> sens;       // (grown to max_batch x the description's n_sensor doubles)
    int feed = 0;              // robots of the feed (0 = no feed)
    Program prog;              // what writes the targets inside a rollout
    Pushes push;               // what pushes the plant inside a rollout
    Walls walls;               // what the EE bodies run into inside a rollout
    Joints joints;             // what acts on single hinges inside a rollout: stops, couplings, drives
    Objects objects;           // what the grippers carry inside a rollout
    Loads loads;               // what the carried objects weigh (only next to the objects they describe)
    Reward reward;             // what judges every tick of a rollout (it reads the other parts; none reads it but the episodes and the log)
    Episodes episodes;         // what ends and restarts single robots inside a rollout
    int ticks_run = 0;         // ticks the last rollout call on the slot ran (fewer than asked: an early exit of its episodes)
    // THE SLOT'S ROLLOUT PARTS, listed three times and nowhere else: a new part goes into all three (adding a part).
    // The model changed: what was laid out for the old one ends -- the compact block and the feed, and every part.
    void model_changed() { drop_block(true); prog.end(); push.end(); walls.end(); joints.end(); objects.end(); loads.end(); reward.end(); episodes.end(); }
    // A whole rollout tick is enqueued (prog_ran: with the program's kernel): every part in force is a tick older.
    void parts_ticked(bool prog_ran) { if (prog_ran) prog.ticked(); push.ticked(); walls.ticked(); joints.ticked(); objects.ticked(); loads.ticked(); episodes.ticked(); }      // (the reward keeps no tick: its steps are per robot)
    // The parts whose state a reset of episodes writes, with the robots each covers: episodes cover no more (irlosc_set_episodes)
    struct Cover { int robots; const char* what; };
    std::array<Cover, 6> reset_covers() const { return {{{prog.robots, "program"}, {walls.robots, "walls"}, {joints.robots, "joint rows"}, {objects.robots, "action objects"}, {loads.robots, "object loads"}, {reward.robots, "reward"}}}; }

    // The feed ends: records that bring a wrench of their own were announced, or its description / the model changed.
    void end_feed() { feed = 0; }
    // The compact block no longer follows the records (and, with `feed_too`, the feed ends): an upload (own wrench) or the front end (none)
    // has named the slot -- before it looks at its other arguments: dropping the block early only costs a re-pack and is never wrong --
    // or the model changed, for which blocks and feeds were laid out.
    void drop_block(bool feed_too) { packed = 0; if (feed_too) end_feed(); }
    // Records are about to be written (arguments validated, no device write yet): nothing usable in the slot until they are accepted,
    // and if they are refused or a copy fails, that is why the slot is empty -- not an earlier fused step.
    void writing() { records = 0; tree = 0; packed = 0; fused_away = 0; }
    // Records of B robots are in the slot: with or without a wrench, and `tree` the verdict on them (1: probed or by construction, 0: not,
    // or unknown).  Also a new verdict on records already there (irlosc_probe_structure).  Their block is packed after this.
    void accepted(int B, bool wrench_, int tree_) { records = B; has_wrench = wrench_; tree = tree_; packed = 0; }
    // An empty batch (B == 0) was uploaded.
    void emptied() { records = -1; tree = 0; packed = 0; }
    // A fused step's give-up pass wrote records of some robots over them: no records, and the error text says why.
    void voided() { records = 0; tree = 0; packed = 0; fused_away = 1; }
    // Records and coordinates (`wrench_too`: and the wrench buffer) are scratch of a device-pointer step: none of it is the slot's state.
    void lent(bool wrench_too) { records = 0; tree = 0; packed = 0; coords = 0; if (wrench_too) has_wrench = 0; }
    // The plant kernel of a rollout advanced the coordinates of B robots on the device: row-major and walk layout alike, so they stay the
    // slot's coordinates (targets and feed are not touched; the records went with the fused step of the tick: voided()).
    void advanced(int B) { coords = B; }
    // irlosc_set_episodes wrote start state 0 of B robots into the coordinates on the device, both layouts: they are the slot's coordinates.
    void restarted(int B) { coords = B; }
    // pack_slot built the block of B robots from records it found eligible (lane_eligible: the tree verdict, so records > 0).
    void block_packed(int B) { packed = B; }
};

// The device arrays a step reads, in the context's dtype (tvel / wrench: nullptr = none; bias: nullptr without IRLOSC_USE_G)
struct StepInputs {
    const void *M, *J, *dq, *bias, *ee, *tgt, *tvel, *wrench;
};

// The one way from a slot to a step's inputs: target velocities only if the slot has them; the wrench `feed_wrench` computed from a
// sensor feed when given, else the records' own if they carry one.
static StepInputs slot_inputs(const Slot& s, const void* feed_wrench = nullptr) {
    return StepInputs{s.M, s.J, s.dq, s.bias, s.ee, s.tgt, s.has_tvel ? s.tvel : nullptr,
                      feed_wrench ? feed_wrench : s.has_wrench ? s.wrench : nullptr};
}

// ... and to the record arrays a front end writes
template <typename T>
static FeOut<T> slot_out(const Slot& s) {
    return FeOut<T>{(T*)s.M.get(), (T*)s.J.get(), (T*)s.dq.get(), (T*)s.bias.get(), (T*)s.ee.get()};
}

// What a model means for the context, planned ON THE HOST by irlosc_set_model (derive_model, then plan_routes: neither touches the
// context's state or the device).  The defaults are the state before the first model: no walk, no fused path, no lane tier, no pack table.
struct ModelPlan {
    FeModel h{};                      // the validated model with its derived tables (the device copy: Model::dmodel)
    size_t fe_smem = 0;               // LDS of the wave-per-robot front end
    int fe_lane = 0;                  // 1: the model has the compiled Dual-UR5 shape -> lane-per-instance front end
    int fe_lane_s = 0;                // 1: ... and the structural constants of its MJCF -> the fused walk with them compiled in (TopoDualUr5S)
    // fused path (irlosc_step_from_q / irlosc_step_resident_from_q on the row16 kernel): entry tables of the compact exchange buffer
    // (one buffer per step of a train: Bank::xside)
    int fused = 0;
    int fq_overlap = 1;               // IRLOSC_FQ_OVERLAP=0: one bank, one stream (A/B measurements, tests)
    FeCompactTables tables{};
    size_t fe_xentries = 0;
    int32_t ft_qe[IRLOSC_MAX_DEV] = {};    // exchange entry of each EE's qw (FeCompactTables::eetab[d][3]): the F/T sensor feed reads it
    // the OSC step of the fused path in lane-per-robot form (osc_lane.hpp): the instantiation that holds the layout (-1: none: the row16
    // FROMQ kernel stays) and its row map
    int lane_tier = -1;
    lane::RowMap lane_map{};
    // resident lane route: the pack table of the layout (pack_plan; pack_ok = 0: none)
    int pack_ok = 0;
    PackTable pack{};

    void plan_routes(const irlosc_ctx* c);
};

// The model of a context: the plan in force with its device copies.  Written by the methods below and by nothing else: commit() is the
// one way a plan becomes the context's, the give_up_*() are the routes a context loses when their buffers cannot be allocated.  While
// `in_force` is 0 the plan is the default one and the entry points from joint coordinates answer IRLOSC_ERR_STATE -- before the first
// irlosc_set_model, and after one that failed on the device (never half of a model).
struct Model : ModelPlan {
    int in_force = 0;
    DevBuf<FeModel> dmodel;
    DevBuf<FeCompactTables> dtables;
    DevBuf<PackTable> dpack;
    DevBuf<int32_t> dpack_bad;        // robots whose dropped entries were not zero (the pack's check)
    DevBuf<double> fe_side;           // side buffer of the lane front end: [wave][entry][64], allocated by the first irlosc_frontend

    int commit(irlosc_ctx* c, const ModelPlan& p);
    // Bank 0 has no exchange buffers: no fused path on this context, the steps from joint coordinates go through dense records.
    void give_up_fused(irlosc_ctx* c);
    // Bank 0 has no lane records: the OSC step of the fused path stays the row16 FROMQ kernel (and no slot takes the resident lane route).
    void give_up_lane(irlosc_ctx* c);
    // No side buffer: the wave-per-robot front end, which needs none, writes the records -- and with the lane walk goes the fused path.
    void give_up_lane_walk() { fe_lane = 0; fused = 0; }
};

struct irlosc_ctx {
    irlosc_cfg cfg{};
    int k = 0;
    size_t esz = 4;
    Stream stream;                     // (declared ahead of everything enqueued on it: destroyed last)
    Stream log_stream;                 // irlosc_rollout_from_q_logged: the stream a half of the log's ring drains on
    Event ev0, ev1;
    std::vector<Slot> slot;            // resident inputs, one set per slot
    int nsets = 1;                     // output sets of bank 0: step i of a row16 train writes set i; the generic path only ever uses set 0
    int train = 1;                     // steps per launch in irlosc_step_resident
    hipEvent_t tev_begin = nullptr, tev_end = nullptr;   // timing events handed to the next train launch (or null)
    DevBuf<unsigned long long> dspan;      // irlosc_time_trains: [ntrains][2] wall-clock stamps written by the kernels, grown on demand
    unsigned long long* span_next = nullptr;   // the pair the next train launch stamps (or null)
    const struct PlantCall* plant_next = nullptr;   // irlosc_rollout_from_q: the plant call the next fused train ends with (or null)
    std::vector<Event> tev_pool;
    void* du = nullptr;                // output set written by the most recent step
    uint32_t* dflags = nullptr;
    DevBuf<unsigned char> draw;        // staging for irlosc_upload_raw (raw simulator arrays), grown on demand
    DevBuf<void> dzeros;               // fp64 row16 path: zero page for the padding lanes
    Model model;                       // rigid-body front end and everything else irlosc_set_model decides
    int task_pass = 1;                     // IRLOSC_TASK_PASS=0: part 1 of the task signal in the row16 kernel (A/B, tests)
    // Consecutive trains of irlosc_step_resident_from_q / irlosc_step_resident rotate over BANKS of buffers, each on a stream of its own:
    // the walk and the lane kernel run one wave per SIMD, eight waves deep per train, so every kernel boundary leaves SIMDs idle for up to
    // a wave's lifetime (~50 us) -- measured as a fixed ~126 us per train of 990 us (trains of 8 / 4 / 2 steps: 124 / 140 / 163 us per
    // step).  With the NEXT trains independent and on other streams their first waves fill those tails (two banks: 60 us of the 126
    // left; three: ~45).  Bank 0 is the context's own, on `stream`: its output sets, give-up lists and counters come with the context
    // (create_impl) and serve single steps too.  The other banks, and every bank's per-step buffers of the task pass, the fused path's
    // exchange buffers and the lane form's records, are allocated by the first call that needs them (ensure_bank).
    struct Bank {
        hipStream_t st = nullptr;          // bank 0: the context's stream; the others: own_st
        Stream own_st;
        Event done;
        DevBuf<void> u[R16_TRAIN];             // output sets
        DevBuf<uint32_t> flags[R16_TRAIN];
        DevBuf<int32_t> list[R16_TRAIN];       // give-up list of each step of a train
        DevBuf<int32_t> count;                 // [R16_TRAIN] give-up counters, zeroed in front of every train
        DevBuf<double> trows[R16_TRAIN];       // dense-record trains: task rows of each step (osc_task_rows_dense_kernel)
        DevBuf<double> xside[R16_TRAIN];       // fused path: compact exchange buffer of each step ...
        size_t xentries = 0;                   // ... sized for this many entries
        DevBuf<double> lane_rec[R16_TRAIN];    // lane form of the fused path: eigen-pass records of each step, and their counters
        DevBuf<int32_t> lane_count;
        DevBuf<void> ftw[R16_TRAIN];           // wrench of each step whose slot has a sensor feed (allocated by the first such step)
    };
    static constexpr int FQ_BANKS = 3;     // banks of the fused path's trains (k13 6.88 -> 7.00e8 against two; four: 7.03e8, +2.4 GB each)
    static constexpr int R16_BANKS = 2;    // banks of the dense-record trains (a third was a cache artefact of a four-slot bench)
    static constexpr int MAX_XBANKS = FQ_BANKS - 1;
    Bank bank[1 + MAX_XBANKS];
    Event ev_join;
    Event ev_dev;                          // irlosc_step_from_q_device: a caller stream starts behind the context's stream
    int r16_overlap = 1;                   // IRLOSC_R16_OVERLAP=0: one bank, one stream for the trains of irlosc_step_resident on dense records
    int32_t* count_cur = nullptr;          // give-up counters of the most recent train (irlosc_giveup_counts)
    // F/T sensor feed of the steps from joint coordinates (irlosc_set_ft_sensors / irlosc_set_sensordata): the description and R_rel
    // per device (the sensordata: Slot::sens; the exchange entries it reads: ModelPlan::ft_qe)
    int ft_set = 0;
    int32_t ft_n_sensor = 0;
    int32_t ft_f0[IRLOSC_MAX_DEV] = {}, ft_t0[IRLOSC_MAX_DEV] = {};
    double ft_R[IRLOSC_MAX_DEV][9] = {};
    // irlosc_tick: one pinned host block and one device block per direction, grown on demand
    PinnedBuf tick_hin, tick_hout;
    DevBuf<unsigned char> tick_din, tick_dout;
    // irlosc_rollout_from_q: the plant in force (irlosc_set_plant), the OR of the ticks' flags, the bounded device buffer of the EE trace
    int plant_set = 0;
    irlosc_plant plant{};
    DevBuf<uint32_t> dflags_any;
    DevBuf<double> dtrace;
    // irlosc_rollout_from_q_logged: the device ring of the episode log (two halves of whole samples), the index list of the logged robots,
    // and per half the pinned block it drains into with its events: `full` on the rollout's stream behind the half's last sample,
    // `drained` on log_stream behind its copy
    DevBuf<double> dlog;
    DevBuf<int32_t> dlog_robots;
    PinnedBuf log_stage[2];
    Event log_full[2], log_drained[2];
    // the early exit of a rollout with episodes: two pinned copies of the running array in turn, each behind its event on the rollout's stream
    PinnedBuf run_stage;
    Event run_copied[2];
    DevBuf<int32_t> dsym;     // symmetry probe of the throughput paths: {count, first instance}
    // Tree-structured factorisation on dense records (row16 kernel), for slots whose records carry the tree's zeros (Slot::tree)
    int tree_enabled = 1;              // IRLOSC_TREE=0 turns the form off (A/B measurements)
    // Resident lane route (irlosc_step / irlosc_step_resident on float64 tree-form records of an AUTO context with a lane tier): the pack
    // pass builds the slot's compact block from the dense records when they enter the slot (Slot::blk, Slot::packed)
    int auto_kernel = 0;               // created with IRLOSC_KERNEL_AUTO
    int resident_lane = 1;             // IRLOSC_RESIDENT_LANE=0 turns the route off (A/B measurements, tests)
    StructureMasks tree_masks;
    DevBuf<int32_t> dstruct;           // result word of the structure probe
    DevBuf<void> dgains;      // [nb][ndev][12] in dtype
    DevBuf<void> dnullkv;     // [nb]
    int gains_nb = 0;
    DevBuf<unsigned long long> ddbg;     // IRLOSC_PHASE_TIMING=1: 8 cycle stamps + 2 wall-clock stamps per stage-1 wave
    int kernel = IRLOSC_KERNEL_GENERIC;
    int kernel_class = IRLOSC_CLASS_GENERIC;
    std::string kernel_name;
    std::string err;
};

static int fail(irlosc_ctx* c, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (c) c->err = buf; else g_create_error = buf;
    return code;
}

#define HIPCHK(c, expr)                                                                          \
    do {                                                                                         \
        hipError_t e_ = (expr);                                                                  \
        if (e_ != hipSuccess)                                                                    \
            return fail((c), IRLOSC_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_));     \
    } while (0)

extern "C" int irlosc_abi_version(void) { return IRLOSC_ABI_VERSION; }

extern "C" int irlosc_device_count(void) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        g_create_error = std::string("hipGetDeviceCount failed: ") + hipGetErrorString(e);
        return IRLOSC_ERR_HIP;
    }
    return n;
}

extern "C" const char* irlosc_last_error(const irlosc_ctx* ctx) {
    return ctx ? ctx->err.c_str() : g_create_error.c_str();
}

extern "C" const char* irlosc_frontend_name(const irlosc_ctx* ctx) {
    if (!ctx || !ctx->model.in_force) return "";
    const bool f64 = ctx->cfg.dtype == IRLOSC_F64;
    if (ctx->model.fe_lane) return f64 ? "osc_frontend_lane_dual_ur5_f64out" : "osc_frontend_lane_dual_ur5_f32out";
    return f64 ? "osc_frontend_generic_f64out" : "osc_frontend_generic_f32out";
}

extern "C" const char* irlosc_kernel_name(const irlosc_ctx* ctx) {
    return ctx ? ctx->kernel_name.c_str() : "";
}
extern "C" int irlosc_kernel_class(const irlosc_ctx* ctx) { return ctx ? ctx->kernel_class : IRLOSC_ERR_ARG; }

static int validate(const irlosc_cfg* c, int* k_out) {
    if (!c) return fail(nullptr, IRLOSC_ERR_ARG, "cfg is NULL");
    if (c->dtype != IRLOSC_F32 && c->dtype != IRLOSC_F64)
        return fail(nullptr, IRLOSC_ERR_ARG, "dtype must be IRLOSC_F32 or IRLOSC_F64");
    if (c->n < 1 || c->n > IRLOSC_MAX_N) return fail(nullptr, IRLOSC_ERR_ARG, "n=%d out of [1,%d]", c->n, IRLOSC_MAX_N);
    if (c->ndev < 1 || c->ndev > IRLOSC_MAX_DEV)
        return fail(nullptr, IRLOSC_ERR_ARG, "ndev=%d out of [1,%d]", c->ndev, IRLOSC_MAX_DEV);
    if (c->max_batch < 1) return fail(nullptr, IRLOSC_ERR_ARG, "max_batch must be >= 1");
    if (c->n_slots < 1) return fail(nullptr, IRLOSC_ERR_ARG, "n_slots must be >= 1");
    int k = 0;
    for (int d = 0; d < c->ndev; ++d) {
        int pc = 0;
        for (int i = 0; i < 6; ++i) pc += c->ctrlr_dof[d][i] ? 1 : 0;
        if (pc != c->dev_rows[d])
            return fail(nullptr, IRLOSC_ERR_ARG, "dev_rows[%d]=%d != popcount(ctrlr_dof)=%d", d, c->dev_rows[d], pc);
        if (c->n < 32 && (c->joint_mask[d] >> c->n))
            return fail(nullptr, IRLOSC_ERR_ARG, "joint_mask[%d] has bits >= n", d);
        if (c->j_idx0[d] < 0) return fail(nullptr, IRLOSC_ERR_ARG, "j_idx0[%d] negative", d);
        k += pc;
    }
    if (k < 1 || k > IRLOSC_MAX_K) return fail(nullptr, IRLOSC_ERR_ARG, "k=%d out of [1,%d]", k, IRLOSC_MAX_K);
    if (c->kernel < IRLOSC_KERNEL_AUTO || c->kernel > IRLOSC_KERNEL_ROW16)
        return fail(nullptr, IRLOSC_ERR_ARG, "unknown kernel id %d", c->kernel);
    *k_out = k;
    return IRLOSC_OK;
}

// What a train needs of its bank beside the output sets, give-up lists and counters (irlosc_ctx::Bank, ensure_bank)
enum : unsigned { NEED_ROWS = 1, NEED_X = 2, NEED_LANE = 4, BANK_ALL = ~0u };

// Frees the buffers of `b` that `what` names: the one place that says which buffers a NEED_* class is.
static void free_bank(irlosc_ctx::Bank& b, unsigned what) {
    for (int i = 0; i < R16_TRAIN; ++i) {
        if (what & NEED_ROWS) b.trows[i].reset();
        if (what & NEED_X) b.xside[i].reset();
        if (what & NEED_LANE) b.lane_rec[i].reset();
    }
    if (what & NEED_LANE) b.lane_count.reset();
}

// The A/B switches of the environment, each read when its comment says (irlosc_create or irlosc_set_model): NAME holds `value` /
// NAME=0 (the feature is off)
static bool env_is(const char* name, const char* value) {
    const char* e = getenv(name);
    return e && !strcmp(e, value);
}
static bool env_off(const char* name) { return env_is(name, "0"); }

static int create_impl(irlosc_ctx* c) {
    const irlosc_cfg& g = c->cfg;
    HIPCHK(nullptr, hipSetDevice(g.hip_device));
    HIPCHK(nullptr, c->stream.ensure());
    HIPCHK(nullptr, c->ev0.ensure());
    HIPCHK(nullptr, c->ev1.ensure());
    const size_t B = (size_t)g.max_batch, n = (size_t)g.n, k = (size_t)c->k, nd = (size_t)g.ndev, e = c->esz;
    c->slot.resize(g.n_slots);
    const struct { DevBuf<void> Slot::*buf; size_t bytes; } resident[] = {
        {&Slot::M, B * n * n * e}, {&Slot::J, B * k * n * e}, {&Slot::dq, B * n * e}, {&Slot::bias, B * n * e},
        {&Slot::ee, B * nd * 7 * e}, {&Slot::wrench, B * nd * 6 * e}, {&Slot::tgt, B * nd * 7 * e}, {&Slot::tvel, B * nd * 6 * e}};
    for (const auto& r : resident)
        for (Slot& s : c->slot) HIPCHK(nullptr, (s.*r.buf).ensure(r.bytes));
    if (c->kernel == IRLOSC_KERNEL_ROW16) {
        c->train = R16_TRAIN;
        c->nsets = R16_TRAIN;               // a train completes (give-up pass included) before the next one starts
    }
    irlosc_ctx::Bank& b0 = c->bank[0];
    b0.st = c->stream;
    for (int k2 = 0; k2 < c->nsets; ++k2) {
        HIPCHK(nullptr, b0.u[k2].ensure(B * n * e));
        HIPCHK(nullptr, b0.flags[k2].ensure(B * sizeof(uint32_t), c->stream));
    }
    if (c->kernel == IRLOSC_KERNEL_ROW16) {
        HIPCHK(nullptr, c->dzeros.ensure(64 * 1024, c->stream));
        for (int k2 = 0; k2 < R16_TRAIN; ++k2) HIPCHK(nullptr, b0.list[k2].ensure(B * sizeof(int32_t)));
        HIPCHK(nullptr, b0.count.ensure(R16_TRAIN * sizeof(int32_t), c->stream));
        // part 1 of the task signal runs as a pass ahead of the row16 kernel (IRLOSC_TASK_PASS=0: in the kernel; A/B, tests); its
        // rows buffers are allocated by the first train that needs them (ensure_bank)
        c->task_pass = !env_off("IRLOSC_TASK_PASS");
        c->r16_overlap = !env_off("IRLOSC_R16_OVERLAP");
    }
    c->du = b0.u[0];
    c->dflags = b0.flags[0];
    c->count_cur = b0.count;
    HIPCHK(nullptr, c->dsym.ensure(2 * sizeof(int32_t)));
    HIPCHK(nullptr, c->dstruct.ensure(sizeof(int32_t)));
    c->resident_lane = !env_off("IRLOSC_RESIDENT_LANE");
    row16_tree_masks(c->tree_masks.mrow, &c->tree_masks.jcols);
    c->tree_enabled = !env_off("IRLOSC_TREE");
    HIPCHK(nullptr, c->dgains.ensure(B * nd * IRLOSC_GAIN_WORDS * e));
    HIPCHK(nullptr, c->dnullkv.ensure(B * e));
    if (c->kernel != IRLOSC_KERNEL_GENERIC && getenv("IRLOSC_PHASE_TIMING"))     // debug aid: cycles per kernel phase
        HIPCHK(nullptr, c->ddbg.ensure((B / 4 + 1) * 10 * sizeof(unsigned long long)));
    HIPCHK(nullptr, hipStreamSynchronize(c->stream));
    return IRLOSC_OK;
}

static bool row16_supported(const irlosc_ctx* c) {
    return row16_kernel_supports(c->cfg.dtype, c->cfg.n, c->k, c->cfg.ndev);
}

extern "C" int irlosc_create(const irlosc_cfg* cfg, irlosc_ctx** out) {
    if (!out) return fail(nullptr, IRLOSC_ERR_ARG, "out is NULL");
    *out = nullptr;
    int k = 0;
    int rc = validate(cfg, &k);
    if (rc) return rc;
    int ndevs = 0;
    if (hipGetDeviceCount(&ndevs) != hipSuccess || ndevs < 1)
        return fail(nullptr, IRLOSC_ERR_HIP, "no HIP device available (libirlosc has no CPU fallback)");
    if (cfg->hip_device < 0 || cfg->hip_device >= ndevs)
        return fail(nullptr, IRLOSC_ERR_ARG, "hip_device=%d but %d device(s) visible", cfg->hip_device, ndevs);
    irlosc_ctx* c = new (std::nothrow) irlosc_ctx();
    if (!c) return fail(nullptr, IRLOSC_ERR_HIP, "out of host memory");
    c->cfg = *cfg;
    c->k = k;
    c->esz = cfg->dtype == IRLOSC_F64 ? 8 : 4;
    if (cfg->kernel == IRLOSC_KERNEL_REMOVED_GROUP) {
        delete c;
        return fail(nullptr, IRLOSC_ERR_ARG, "kernel id 2 (the fp32-arithmetic group kernel of ABI versions 1-2) was removed in ABI version 3: its error is "
                    "eps32 * cond(J M^-1 J^T), 14 %% of physical instances missed the 1e-5 contract; float32 RECORDS run on IRLOSC_KERNEL_AUTO (fp64 arithmetic)");
    }
    if (cfg->kernel == IRLOSC_KERNEL_ROW16 && !row16_supported(c)) {
        delete c;
        return fail(nullptr, IRLOSC_ERR_ARG, "row16 kernel not available for dtype=%d n=%d k=%d ndev=%d", cfg->dtype, cfg->n, k, cfg->ndev);
    }
    // Every kernel computes in fp64 (the reference's arithmetic, and what north_star's 1e-5 needs).  AUTO = the row16 kernel where the
    // shape has one -- on float64 records, and on float32 records too (the "mixed" path: fp32 storage, fp64 arithmetic) -- else the
    // generic kernel.
    c->kernel = IRLOSC_KERNEL_GENERIC;
    c->auto_kernel = cfg->kernel == IRLOSC_KERNEL_AUTO;
    if (cfg->kernel == IRLOSC_KERNEL_ROW16) c->kernel = IRLOSC_KERNEL_ROW16;
    else if (cfg->kernel == IRLOSC_KERNEL_AUTO && row16_supported(c)) c->kernel = IRLOSC_KERNEL_ROW16;
    char nm[96];
    const bool mixed = c->kernel == IRLOSC_KERNEL_ROW16 && cfg->dtype == IRLOSC_F32;
    snprintf(nm, sizeof nm, "%s_%s_n%d_k%d",
             c->kernel == IRLOSC_KERNEL_ROW16 ? "osc_row16" : "osc_generic",
             mixed ? "f32in_f64" : cfg->dtype == IRLOSC_F64 ? "f64" : "f32", cfg->n, k);
    c->kernel_name = nm;
    c->kernel_class = c->kernel == IRLOSC_KERNEL_GENERIC ? IRLOSC_CLASS_GENERIC
                      : row16_kernel_exact(cfg->n, k, cfg->ndev) ? IRLOSC_CLASS_ROW16 : IRLOSC_CLASS_ROW16_PADDED;
    if (c->kernel_class == IRLOSC_CLASS_ROW16_PADDED) {      // the tier the launches will pick (tu_row16_pad_impl.hpp)
        snprintf(nm, sizeof nm, "_ndev%d_pad%d", cfg->ndev, row16_pad_tier(k));
        c->kernel_name += nm;
    }
    rc = create_impl(c);
    if (rc) {
        delete c;      // (its owners release what was allocated: the device is current, set by create_impl's first line)
        return rc;
    }
    *out = c;
    return IRLOSC_OK;
}

extern "C" void irlosc_destroy(irlosc_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->cfg.hip_device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    delete c;
}

template <typename T>
static void convert(const double* src, std::vector<unsigned char>& dst, size_t count) {
    dst.resize(count * sizeof(T));
    T* d = reinterpret_cast<T*>(dst.data());
    for (size_t i = 0; i < count; ++i) d[i] = (T)src[i];
}

extern "C" int irlosc_set_gains(irlosc_ctx* c, const double* gains, const double* null_kv, int32_t nb) {
    if (!c) return IRLOSC_ERR_ARG;
    if (!gains) return fail(c, IRLOSC_ERR_ARG, "gains is NULL");
    if (nb != 1 && nb != c->cfg.max_batch)
        return fail(c, IRLOSC_ERR_ARG, "nb must be 1 (broadcast) or max_batch=%d, got %d", c->cfg.max_batch, nb);
    if ((c->cfg.flags & IRLOSC_NULLSPACE) && !null_kv)
        return fail(c, IRLOSC_ERR_ARG, "null_kv required with IRLOSC_NULLSPACE");
    HIPCHK(c, hipSetDevice(c->cfg.hip_device));
    const size_t cnt = (size_t)nb * c->cfg.ndev * IRLOSC_GAIN_WORDS;
    std::vector<double> zero(nb, 0.0);
    const double* nk = null_kv ? null_kv : zero.data();
    std::vector<unsigned char> a, b;
    if (c->cfg.dtype == IRLOSC_F64) { convert<double>(gains, a, cnt); convert<double>(nk, b, nb); }
    else { convert<float>(gains, a, cnt); convert<float>(nk, b, nb); }
    HIPCHK(c, hipMemcpyAsync(c->dgains, a.data(), a.size(), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->dnullkv, b.data(), b.size(), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->gains_nb = nb;
    for (Slot& s : c->slot) {      // their gain copies were made from the gains this call replaced (and episodes go with the list they reset)
        if (s.prog.kind == Program::LIST) s.episodes.end();
        s.prog.end(Program::LIST);
    }
    return IRLOSC_OK;
}

static int check_slot(irlosc_ctx* c, int slot, int B) {
    if (slot < 0 || slot >= c->cfg.n_slots) return fail(c, IRLOSC_ERR_ARG, "slot %d out of [0,%d)", slot, c->cfg.n_slots);
    if (B < 0 || B > c->cfg.max_batch) return fail(c, IRLOSC_ERR_ARG, "B=%d out of [0,%d]", B, c->cfg.max_batch);
    return IRLOSC_OK;
}

// The throughput kernels read row j of M as its column j (include/irlosc.h, contracts): an asymmetric M would give a wrong
// answer without any flag, so records that come from the HOST are checked before they are accepted (the generic kernel uses
// M as given, like osc.py:49,151, and takes anything).  Small batches on the host, on the caller's own array (B = 1: under a
// microsecond, no kernel in the tick); large ones on the device, one pass over M behind the copy.
static constexpr int SYM_HOST_MAX_B = 32;
static bool sym_applies(const irlosc_ctx* c) { return c->kernel != IRLOSC_KERNEL_GENERIC; }

template <typename T>
static int symmetry_host_t(irlosc_ctx* c, const T* M, int B) {
    const int n = c->cfg.n;
    for (int b = 0; b < B; ++b) {
        const T* Mb = M + (size_t)b * n * n;
        double asym = 0.0, scale = 0.0;
        for (int i = 0; i < n; ++i)
            for (int j = 0; j < n; ++j) {
                const double v = (double)Mb[i * n + j], w = (double)Mb[j * n + i];
                if (!std::isfinite(v) || !std::isfinite(w)) continue;      // a diverged robot is the kernel's business (per-instance flags)
                asym = std::max(asym, std::fabs(v - w));
                scale = std::max(scale, std::fabs(v));
            }
        if (asym > 1e-6 * std::max(scale, 1e-300))
            return fail(c, IRLOSC_ERR_ARG, "M of instance %d is not symmetric (max |M - M^T| = %.3g): the %s kernel reads rows of M as "
                        "columns; use IRLOSC_KERNEL_GENERIC for a non-symmetric M", b, asym, c->kernel_name.c_str());
    }
    return IRLOSC_OK;
}
static int symmetry_host(irlosc_ctx* c, const void* M, int B) {
    return c->cfg.dtype == IRLOSC_F64 ? symmetry_host_t<double>(c, (const double*)M, B) : symmetry_host_t<float>(c, (const float*)M, B);
}
// Device probe: zeroes the two result words at `dres` and enqueues the pass; the caller brings them back with whatever copy
// it makes anyway and hands them to symmetry_verdict.
static int symmetry_probe(irlosc_ctx* c, const void* dM, int B, int32_t* dres, hipStream_t st) {
    HIPCHK(c, hipMemsetAsync(dres, 0, 2 * sizeof(int32_t), st));
    const int rc = c->cfg.dtype == IRLOSC_F64 ? launch_symmetry_probe<double>((const double*)dM, c->cfg.n, B, dres, st)
                                              : launch_symmetry_probe<float>((const float*)dM, c->cfg.n, B, dres, st);
    HIPCHK(c, (hipError_t)rc);
    return IRLOSC_OK;
}
static int symmetry_verdict(irlosc_ctx* c, const int32_t res[2]) {
    if (res[0] > 0)
        return fail(c, IRLOSC_ERR_ARG, "M of instance %d is not symmetric (%d instance(s) with max |M - M^T| > 1e-6 max |M|): the %s "
                    "kernel reads rows of M as columns; use IRLOSC_KERNEL_GENERIC for a non-symmetric M", 0x7fffffff - res[1], res[0],
                    c->kernel_name.c_str());
    return IRLOSC_OK;
}

// the tree-structured form of the row16 kernel applies to the records of this slot
static bool slot_tree(const irlosc_ctx* c, int slot) {
    return c->tree_enabled && c->kernel == IRLOSC_KERNEL_ROW16 && c->slot[slot].tree != 0;
}

// Zero pattern of the records in a slot (synchronous; a throughput feature: batches under 64 instances keep the dense form).
// The pattern is that of the compiled Dual-UR5 tree, so the question only arises for its shape (n = 25).
static int pack_slot(irlosc_ctx* c, int slot, int B, bool check);

// -> *tree: the verdict on the first B records in the slot (0 where the question does not arise, and on failure)
static int structure_probe(irlosc_ctx* c, const Slot& s, int B, int* tree) {
    *tree = 0;
    if (!c->tree_enabled || c->kernel != IRLOSC_KERNEL_ROW16 || B < 64) return IRLOSC_OK;
    int32_t bad = 0;
    HIPCHK(c, hipMemsetAsync(c->dstruct, 0, sizeof(int32_t), c->stream));
    const int rc = c->cfg.dtype == IRLOSC_F64
        ? launch_structure_probe<double>((const double*)s.M.get(), (const double*)s.J.get(), c->cfg.n, c->k, B, c->tree_masks, c->dstruct, c->stream)
        : launch_structure_probe<float>((const float*)s.M.get(), (const float*)s.J.get(), c->cfg.n, c->k, B, c->tree_masks, c->dstruct, c->stream);
    HIPCHK(c, (hipError_t)rc);
    HIPCHK(c, hipMemcpyAsync(&bad, c->dstruct, sizeof bad, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *tree = bad == 0;
    return IRLOSC_OK;
}

// Shared head of the four upload entry points, right after check_slot.  -> true: an empty batch, the call is done.
static bool upload_head(Slot& s, int B) {
    s.drop_block(true);      // records bring a wrench of their own: the slot's sensor feed ends here (and the compact block follows the
                             // records: rebuilt from the new ones)
    if (B == 0) s.emptied();
    return B == 0;
}

// Shared tail of the four upload entry points, the records of B robots written and (from the host) found symmetric: the slot holds them.
// `probe`: they were written on the context's stream and it has drained, so their zero pattern is looked at (synchronous) and
// tree-form records of a lane-route slot get their compact block; else the verdict is unknown (irlosc_probe_structure: and the block).
static int upload_tail(irlosc_ctx* c, int slot, int B, bool has_wrench, bool probe) {
    Slot& s = c->slot[slot];
    int tree = 0;
    if (probe) {
        const int rc = structure_probe(c, s, B, &tree);
        if (rc) return rc;
    }
    s.accepted(B, has_wrench, tree);
    return probe ? pack_slot(c, slot, B, true) : IRLOSC_OK;
}

extern "C" int irlosc_probe_structure(irlosc_ctx* c, int32_t slot, int32_t B) {
    if (!c) return IRLOSC_ERR_ARG;
    int rc = check_slot(c, slot, B);
    if (rc) return rc;
    Slot& s = c->slot[slot];
    if (B > std::max(0, s.records))
        return fail(c, IRLOSC_ERR_STATE, "slot %d holds records of %d instances, probe asked for %d", slot, std::max(0, s.records), B);
    HIPCHK(c, hipSetDevice(c->cfg.hip_device));
    int tree = 0;
    rc = structure_probe(c, s, B, &tree);
    s.accepted(s.records, s.has_wrench, tree);      // the same records under a new verdict (none, if the probe failed)
    if (!rc) rc = pack_slot(c, slot, B, true);
    if (rc) return rc;
    return slot_tree(c, slot) ? 1 : 0;
}

extern "C" int irlosc_slot_structure(const irlosc_ctx* c, int32_t slot) {
    if (!c || slot < 0 || slot >= c->cfg.n_slots) return 0;
    return slot_tree(c, slot) ? 1 : 0;
}

static int record_route(const irlosc_ctx* c, int slot, int B);

extern "C" int irlosc_slot_route(const irlosc_ctx* c, int32_t slot, int32_t B) {
    if (!c || slot < 0 || slot >= c->cfg.n_slots) return IRLOSC_ROUTE_NONE;
    return record_route(c, slot, B > 0 ? B : std::max(0, c->slot[slot].records));
}

extern "C" int irlosc_upload(irlosc_ctx* c, int32_t slot, int32_t B, const void* M, const void* J, const void* dq,
                             const void* bias, const void* ee_pose, const void* wrench) {
    if (!c) return IRLOSC_ERR_ARG;
    int rc = check_slot(c, slot, B);
    if (rc) return rc;
    Slot& s = c->slot[slot];
    if (upload_head(s, B)) return IRLOSC_OK;
    if (!M || !J || !dq || !ee_pose) return fail(c, IRLOSC_ERR_ARG, "M, J, dq and ee_pose are required");
    if ((c->cfg.flags & IRLOSC_USE_G) && !bias) return fail(c, IRLOSC_ERR_ARG, "bias required with IRLOSC_USE_G");
    HIPCHK(c, hipSetDevice(c->cfg.hip_device));
    const size_t b = (size_t)B, n = (size_t)c->cfg.n, k = (size_t)c->k, nd = (size_t)c->cfg.ndev, e = c->esz;
    s.writing();
    HIPCHK(c, hipMemcpyAsync(s.M, M, b * n * n * e, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(s.J, J, b * k * n * e, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(s.dq, dq, b * n * e, hipMemcpyHostToDevice, c->stream));
    if (bias) HIPCHK(c, hipMemcpyAsync(s.bias, bias, b * n * e, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(s.ee, ee_pose, b * nd * 7 * e, hipMemcpyHostToDevice, c->stream));
    if (wrench) HIPCHK(c, hipMemcpyAsync(s.wrench, wrench, b * nd * 6 * e, hipMemcpyHostToDevice, c->stream));
    if (sym_applies(c)) {
        int rcs;
        if (B <= SYM_HOST_MAX_B) {
            rcs = symmetry_host(c, M, B);
        } else {
            int32_t res[2] = {0, 0};
            rcs = symmetry_probe(c, s.M, B, c->dsym, c->stream);
            if (rcs) return rcs;
            HIPCHK(c, hipMemcpyAsync(res, c->dsym, sizeof res, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            rcs = symmetry_verdict(c, res);
        }
        if (rcs) return rcs;
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return upload_tail(c, slot, B, wrench != nullptr, true);
}

// Enqueue the assembly kernel: dptr = device pointers {qM, qvel, qfrc_bias, jacp, jacr, ee_xpos, ee_xquat, site_xmat, sensordata}.
template <typename T>
static int assemble_launch(irlosc_ctx* c, const Slot& s, int B, const irlosc_raw_desc* rd, const void* const* dptr, hipStream_t st,
                           const irlosc_qm_layout* qml = nullptr) {
    RawDesc d;
    memset(&d, 0, sizeof d);
    if (qml) {
        d.nM = qml->nM;
        for (int j = 0; j < IRLOSC_MAX_NV; ++j) d.pos[j] = -1;
        for (int j = 0; j < rd->nv; ++j) { d.madr[j] = (int16_t)qml->dof_Madr[j]; d.par[j] = (int16_t)qml->dof_parentid[j]; }
        for (int i = 0; i < c->cfg.n; ++i) d.pos[rd->joint_ids[i]] = (int16_t)i;
    }
    d.nv = rd->nv; d.n_sensor = rd->n_sensor; d.n = c->cfg.n; d.k = c->k; d.ndev = c->cfg.ndev;
    for (int i = 0; i < c->cfg.n; ++i) { d.joint_ids[i] = rd->joint_ids[i]; d.dq_src[i] = rd->dq_src[i]; }
    for (int dv = 0; dv < c->cfg.ndev; ++dv) {
        d.ft_force0[dv] = rd->ft_force0[dv]; d.ft_torque0[dv] = rd->ft_torque0[dv];
        for (int i = 0; i < 6; ++i) if (c->cfg.ctrlr_dof[dv][i]) d.dofmask[dv] |= 1u << i;
    }
    const bool ft = dptr[7] && dptr[8] && rd->n_sensor > 0;
    RawPtrs<T> r;
    r.qM = (const T*)dptr[0]; r.qvel = (const T*)dptr[1]; r.qfrc_bias = (const T*)dptr[2];
    r.jacp = (const T*)dptr[3]; r.jacr = (const T*)dptr[4]; r.ee_xpos = (const T*)dptr[5]; r.ee_xquat = (const T*)dptr[6];
    r.site_xmat = ft ? (const T*)dptr[7] : nullptr; r.sensordata = ft ? (const T*)dptr[8] : nullptr;
    const FeOut<T> o = slot_out<T>(s);
    r.M = o.M; r.J = o.J; r.dq = o.dq; r.bias = o.bias; r.ee = o.ee; r.wrench = (T*)s.wrench.get();
    HIPCHK(c, (hipError_t)launch_assemble<T>(d, r, B, st));
    return IRLOSC_OK;
}

static int check_raw_desc(irlosc_ctx* c, const irlosc_raw_desc* rd) {
    if (rd->nv < 1 || rd->n_sensor < 0) return fail(c, IRLOSC_ERR_ARG, "bad nv / n_sensor");
    for (int i = 0; i < c->cfg.n; ++i) {
        if (rd->joint_ids[i] < 0 || rd->joint_ids[i] >= rd->nv) return fail(c, IRLOSC_ERR_ARG, "joint_ids[%d] out of [0,nv)", i);
        if (rd->dq_src[i] >= rd->nv) return fail(c, IRLOSC_ERR_ARG, "dq_src[%d] out of range", i);
    }
    for (int dv = 0; dv < c->cfg.ndev; ++dv) {
        const int f0 = rd->ft_force0[dv], t0 = rd->ft_torque0[dv];
        if ((f0 >= 0 && f0 + 3 > rd->n_sensor) || (t0 >= 0 && t0 + 3 > rd->n_sensor))
            return fail(c, IRLOSC_ERR_ARG, "F/T sensor slice of device %d exceeds n_sensor", dv);
    }
    return IRLOSC_OK;
}

template <typename T>
static int upload_raw_t(irlosc_ctx* c, const Slot& s, int B, const irlosc_raw_desc* rd, const void* const* src, const irlosc_qm_layout* qml) {
    const size_t b = (size_t)B, nv = (size_t)rd->nv, nd = (size_t)c->cfg.ndev, ns = (size_t)rd->n_sensor, e = sizeof(T);
    const bool ft = src[7] && src[8] && ns > 0;
    // staging layout: qM (dense nv x nv, or MuJoCo's nM-entry form) | qvel | qfrc_bias | jacp | jacr | ee_xpos | ee_xquat | site_xmat | sensordata
    const size_t sz[9] = {qml ? b * (size_t)qml->nM * e : b * nv * nv * e, b * nv * e, b * nv * e, b * nd * 3 * nv * e, b * nd * 3 * nv * e,
                          b * nd * 3 * e, b * nd * 4 * e, ft ? b * nd * 9 * e : 0, ft ? b * ns * e : 0};
    size_t off[9], total = 0;
    for (int i = 0; i < 9; ++i) { off[i] = total; total += (sz[i] + 255) & ~(size_t)255; }
    HIPCHK(c, c->draw.reserve(total));
    unsigned char* base = c->draw;
    for (int i = 0; i < 9; ++i)
        if (sz[i]) HIPCHK(c, hipMemcpyAsync(base + off[i], src[i], sz[i], hipMemcpyHostToDevice, c->stream));
    const void* dptr[9];
    for (int i = 0; i < 9; ++i) dptr[i] = sz[i] ? (const void*)(base + off[i]) : nullptr;
    int rc = assemble_launch<T>(c, s, B, rd, dptr, c->stream, qml);
    if (rc) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return IRLOSC_OK;
}

// MuJoCo's own form of M: validate the layout (every run stays inside [0, nM), the tree is a forest numbered parents first)
static int check_qm_layout(irlosc_ctx* c, const irlosc_raw_desc* rd, const irlosc_qm_layout* q) {
    if (rd->nv > IRLOSC_MAX_NV) return fail(c, IRLOSC_ERR_ARG, "nv=%d exceeds IRLOSC_MAX_NV=%d", rd->nv, IRLOSC_MAX_NV);
    if (q->nM < rd->nv || q->nM > 32767) return fail(c, IRLOSC_ERR_ARG, "nM=%d out of range for nv=%d", q->nM, rd->nv);
    for (int i = 0; i < rd->nv; ++i) {
        if (q->dof_parentid[i] >= i || q->dof_parentid[i] < -1) return fail(c, IRLOSC_ERR_ARG, "dof_parentid[%d]=%d: a parent precedes its child (or is -1)", i, q->dof_parentid[i]);
        int len = 0;
        for (int j = i; j >= 0; j = q->dof_parentid[j]) ++len;
        if (q->dof_Madr[i] < 0 || q->dof_Madr[i] + len > q->nM) return fail(c, IRLOSC_ERR_ARG, "dof_Madr[%d]=%d + %d entries exceeds nM=%d", i, q->dof_Madr[i], len, q->nM);
    }
    return IRLOSC_OK;
}

// What the three raw entry points share behind their own argument checks: the description checked, then the records of B robots
// assembled into the slot from src = {qM, qvel, qfrc_bias, jacp, jacr, ee_xpos, ee_xquat, site_xmat, sensordata} -- host arrays through
// the staging block on the context's stream (st == nullptr; synchronous, and probed: the expansion of `qml` mirrors every entry, the
// dense form is the caller's), or device arrays on `st` (enqueued: no synchronous look at what it writes).
static int raw_records(irlosc_ctx* c, int slot, int B, const irlosc_raw_desc* rd, const irlosc_qm_layout* qml, const void* const* src, hipStream_t st) {
    int rc = check_raw_desc(c, rd);
    if (!rc && qml) rc = check_qm_layout(c, rd, qml);
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->cfg.hip_device));
    Slot& s = c->slot[slot];
    s.writing();
    if (c->cfg.dtype == IRLOSC_F64) rc = st ? assemble_launch<double>(c, s, B, rd, src, st) : upload_raw_t<double>(c, s, B, rd, src, qml);
    else rc = st ? assemble_launch<float>(c, s, B, rd, src, st) : upload_raw_t<float>(c, s, B, rd, src, qml);
    if (rc) return rc;
    return upload_tail(c, slot, B, true, st == nullptr);
}

extern "C" int irlosc_upload_raw_sparse(irlosc_ctx* c, int32_t slot, int32_t B, const irlosc_raw_desc* rd, const irlosc_qm_layout* qml,
                                        const void* qM, const void* qvel, const void* qfrc_bias, const void* jacp, const void* jacr,
                                        const void* ee_xpos, const void* ee_xquat, const void* site_xmat, const void* sensordata) {
    if (!c) return IRLOSC_ERR_ARG;
    int rc = check_slot(c, slot, B);
    if (rc) return rc;
    if (upload_head(c->slot[slot], B)) return IRLOSC_OK;
    if (!rd || !qml || !qM || !qvel || !qfrc_bias || !jacp || !jacr || !ee_xpos || !ee_xquat)
        return fail(c, IRLOSC_ERR_ARG, "desc, qm layout, qM, qvel, qfrc_bias, jacp, jacr, ee_xpos and ee_xquat are required");
    const void* src[9] = {qM, qvel, qfrc_bias, jacp, jacr, ee_xpos, ee_xquat, site_xmat, sensordata};
    return raw_records(c, slot, B, rd, qml, src, nullptr);
}

extern "C" int irlosc_upload_raw(irlosc_ctx* c, int32_t slot, int32_t B, const irlosc_raw_desc* rd, const void* qM,
                                 const void* qvel, const void* qfrc_bias, const void* jacp, const void* jacr,
                                 const void* ee_xpos, const void* ee_xquat, const void* site_xmat,
                                 const void* sensordata) {
    if (!c) return IRLOSC_ERR_ARG;
    int rc = check_slot(c, slot, B);
    if (rc) return rc;
    if (upload_head(c->slot[slot], B)) return IRLOSC_OK;
    if (!rd || !qM || !qvel || !qfrc_bias || !jacp || !jacr || !ee_xpos || !ee_xquat)
        return fail(c, IRLOSC_ERR_ARG, "desc, qM, qvel, qfrc_bias, jacp, jacr, ee_xpos and ee_xquat are required");
    const void* src[9] = {qM, qvel, qfrc_bias, jacp, jacr, ee_xpos, ee_xquat, site_xmat, sensordata};
    return raw_records(c, slot, B, rd, nullptr, src, nullptr);
}

extern "C" int irlosc_assemble_device(irlosc_ctx* c, int32_t slot, int32_t B, const irlosc_raw_desc* rd, const void* qM,
                                      const void* qvel, const void* qfrc_bias, const void* jacp, const void* jacr,
                                      const void* ee_xpos, const void* ee_xquat, const void* site_xmat,
                                      const void* sensordata, void* hip_stream) {
    if (!c) return IRLOSC_ERR_ARG;
    int rc = check_slot(c, slot, B);
    if (rc) return rc;
    if (upload_head(c->slot[slot], B)) return IRLOSC_OK;
    if (!rd || !qM || !qvel || !qfrc_bias || !jacp || !jacr || !ee_xpos || !ee_xquat)
        return fail(c, IRLOSC_ERR_ARG, "desc, qM, qvel, qfrc_bias, jacp, jacr, ee_xpos and ee_xquat are required");
    const void* src[9] = {qM, qvel, qfrc_bias, jacp, jacr, ee_xpos, ee_xquat, site_xmat, sensordata};
    return raw_records(c, slot, B, rd, nullptr, src, hip_stream ? (hipStream_t)hip_stream : c->stream);
}

extern "C" int irlosc_set_targets(irlosc_ctx* c, int32_t slot, int32_t B, const void* tgt_pose, const void* tgt_vel) {
    if (!c) return IRLOSC_ERR_ARG;
    int rc = check_slot(c, slot, B);
    if (rc) return rc;
    Slot& s = c->slot[slot];
    if (B == 0) { s.targets = -1; s.prog.end(); s.episodes.end(); return IRLOSC_OK; }
    if (!tgt_pose) return fail(c, IRLOSC_ERR_ARG, "tgt_pose is NULL");
    s.prog.end();      // the targets are the caller's from here on: one entry point writes them at a time
    s.episodes.end();  // (their snapshot of the targets is stale)
    HIPCHK(c, hipSetDevice(c->cfg.hip_device));
    const size_t b = (size_t)B, nd = (size_t)c->cfg.ndev, e = c->esz;
    HIPCHK(c, hipMemcpyAsync(s.tgt, tgt_pose, b * nd * 7 * e, hipMemcpyHostToDevice, c->stream));
    if (tgt_vel) HIPCHK(c, hipMemcpyAsync(s.tvel, tgt_vel, b * nd * 6 * e, hipMemcpyHostToDevice, c->stream));
    s.has_tvel = tgt_vel != nullptr;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    s.targets = B;
    return IRLOSC_OK;
}

template <typename T>
static void fill_params(const irlosc_ctx* c, KParams<T>& p, int B, const StepInputs& in, void* u, uint32_t* flags) {
    memset(&p, 0, sizeof p);
    p.M = (const T*)in.M; p.J = (const T*)in.J; p.dq = (const T*)in.dq; p.bias = (const T*)in.bias;
    p.ee = (const T*)in.ee; p.tgt = (const T*)in.tgt; p.tvel = (const T*)in.tvel; p.wrench = (const T*)in.wrench;
    p.u = (T*)u; p.flags = flags;
    p.gains = (const T*)c->dgains.get(); p.null_kv = (const T*)c->dnullkv.get();
    p.index = nullptr;
    p.dbg = c->ddbg;
    p.gains_per_instance = c->gains_nb > 1;
    p.B = B; p.n = c->cfg.n; p.k = c->k; p.ndev = c->cfg.ndev; p.cfgflags = c->cfg.flags;
    p.padded = c->kernel_class == IRLOSC_CLASS_ROW16_PADDED ? 1 : 0;      // decided once, at irlosc_create (IRLOSC_FORCE_PAD is read there)
    int row = 0;
    for (int d = 0; d < c->cfg.ndev; ++d) {
        DevMeta& m = p.dev[d];
        m.row0 = row; m.rows = c->cfg.dev_rows[d]; row += m.rows;
        m.dofmask = 0;
        for (int i = 0; i < 6; ++i) if (c->cfg.ctrlr_dof[d][i]) m.dofmask |= 1u << i;
        m.calc = (c->cfg.calc_xyz[d] ? 1u : 0u) | (c->cfg.calc_abg[d] ? 2u : 0u);
        m.joint_mask = c->cfg.joint_mask[d];
        m.jidx0 = c->cfg.j_idx0[d];
    }
}

// An owner's ensure() / reserve() gave what was asked for (else: out of device memory, and the caller decides what follows)
static bool got(hipError_t e) { return e == hipSuccess; }

// Bank k ready for trains of up to n steps that need `need`: task rows (8 MB per step at 65 536 instances), exchange buffers (334 entries
// x 512 B per 64 robots: 175 MB per step), lane records (one per robot and step for the eigen pass, whole groups of 64: all of a batch may
// be flagged) -- and, beside bank 0, the bank's own stream, event, output sets, give-up lists and counters.  Allocated on first use and
// kept, so a context pays only for the trains it runs.  -> 0, or what could not be allocated (BANK_ALL: the bank's own buffers); the
// caller decides what follows.
static unsigned ensure_bank(irlosc_ctx* c, int k, int n, unsigned need) {
    irlosc_ctx::Bank& b = c->bank[k];
    const size_t Bm = (size_t)c->cfg.max_batch, waves = (Bm + 63) / 64;
    if (k > 0) {
        bool ok = got(b.own_st.ensure()) && got(b.done.ensure(hipEventDisableTiming)) && got(c->ev_join.ensure(hipEventDisableTiming)) &&
                  got(b.count.ensure(R16_TRAIN * sizeof(int32_t)));
        b.st = b.own_st;
        for (int i = 0; ok && i < n; ++i)
            ok = got(b.list[i].ensure(Bm * sizeof(int32_t))) && got(b.u[i].ensure(Bm * c->cfg.n * c->esz)) && got(b.flags[i].ensure(Bm * sizeof(uint32_t)));
        if (!ok) { (void)hipGetLastError(); return BANK_ALL; }
    }
    if (need & NEED_ROWS)
        for (int i = 0; i < n; ++i) if (!got(b.trows[i].ensure(Bm * 16 * sizeof(double)))) return NEED_ROWS;
    if (need & NEED_X) {
        if (b.xentries != c->model.fe_xentries) free_bank(b, NEED_X);          // sized for another model's entries
        b.xentries = c->model.fe_xentries;
        for (int i = 0; i < n; ++i) if (!got(b.xside[i].ensure(waves * b.xentries * 64 * sizeof(double)))) return NEED_X;
    }
    if (need & NEED_LANE) {
        if (!got(b.lane_count.ensure(R16_TRAIN * sizeof(int32_t)))) return NEED_LANE;
        for (int i = 0; i < n; ++i) if (!got(b.lane_rec[i].ensure(waves * 64 * lane::REC_DOUBLES * sizeof(double), c->stream))) return NEED_LANE;
    }
    return 0;
}

// Bytes of a coordinate buffer in the fused walk's layout [walk wave][2 n][64 robots] (Slot::qt, Slot::blk_dq)
static size_t qt_bytes(const irlosc_ctx* c) { return (((size_t)c->cfg.max_batch + 63) / 64) * 2 * c->cfg.n * 64 * sizeof(double); }

// Resident lane route: records of at least this many robots qualify (a smaller batch keeps the row16 kernel: irlosc_tick at B = 1 pays
// for no pack)
static constexpr int LANE_MIN_B = 4096;

// Records of B robots in the slot may take the lane route: AUTO context, float64 records, the tree verdict, a model whose layout has a
// lane tier and a pack table, IRLOSC_RESIDENT_LANE not 0
static bool lane_eligible(const irlosc_ctx* c, int slot, int B) {
    return c->resident_lane && c->auto_kernel && c->cfg.dtype == IRLOSC_F64 && c->kernel == IRLOSC_KERNEL_ROW16 && c->model.lane_tier >= 0 &&
           c->model.pack_ok && slot_tree(c, slot) && B >= LANE_MIN_B;
}

// THE route of a step of B robots on the slot's records (IRLOSC_ROUTE_*): what irlosc_slot_route reports is what launch_slot and
// dense_train launch.  The lane route needs a block that follows the records and no target velocities (those: the row16 kernel, as on
// the fused path).
static int record_route(const irlosc_ctx* c, int slot, int B) {
    if (c->kernel != IRLOSC_KERNEL_ROW16) return IRLOSC_ROUTE_GENERIC;
    const Slot& s = c->slot[slot];
    if (B > 0 && s.packed >= B && !s.has_tvel && lane_eligible(c, slot, B)) return IRLOSC_ROUTE_LANE;
    return slot_tree(c, slot) ? IRLOSC_ROUTE_ROW16_TREE : IRLOSC_ROUTE_ROW16;
}
// ... and the route that is left when the lane route's bank records cannot be allocated, or a sensor feed brings the wrench
static int row16_route(int route) { return route == IRLOSC_ROUTE_LANE ? IRLOSC_ROUTE_ROW16_TREE : route; }

// The form of a step from joint coordinates (`tvel`: with target velocities): through dense records (front end, then record_route),
// or fused -- the walk into the compact exchange buffer, then the row16 FROMQ kernel or the lane-per-robot OSC step (not with target
// velocities: branch B of osc.py:173-177 reads dx between the two halves of the task signal).
enum FromQ { FROMQ_DENSE, FROMQ_ROW16, FROMQ_LANE };
static FromQ from_q_form(const irlosc_ctx* c, bool tvel) {
    return !c->model.fused ? FROMQ_DENSE : c->model.lane_tier >= 0 && !tvel ? FROMQ_LANE : FROMQ_ROW16;
}
// What a fused train needs of its bank
static unsigned fused_need(const irlosc_ctx* c) { return NEED_X | (from_q_form(c, false) == FROMQ_LANE ? NEED_LANE : 0); }
// The walk of the fused path: its launcher and the name irlosc_from_q_name reports
struct Walk {
    int (*launch)(const FeModel* dmodel, const FeLaneTrain& tr, int nsteps, hipStream_t st);
    const char* name;
};
static Walk fused_walk(const irlosc_ctx* c) {
    return c->model.fe_lane_s ? Walk{launch_frontend_lane_compact_dual_ur5_s, "osc_frontend_lane_compact_dual_ur5_s"}
                              : Walk{launch_frontend_lane_compact_dual_ur5, "osc_frontend_lane_compact_dual_ur5"};
}

void Model::give_up_fused(irlosc_ctx* c) { free_bank(c->bank[0], NEED_X); fused = 0; }
void Model::give_up_lane(irlosc_ctx* c) { free_bank(c->bank[0], NEED_LANE); lane_tier = -1; }

// The compact block of the slot's records of B robots, on the context's stream behind whatever wrote them.  `check`: the pack counts the
// robots whose dropped entries are not zero and the block is only valid without one (synchronous; the record-form front end writes the
// tree's zeros by construction and needs no check).  Out of device memory: no block, the slot keeps the row16 route.
// Called behind accepted(), which has dropped the block of the records before.
static int pack_slot(irlosc_ctx* c, int slot, int B, bool check) {
    Slot& s = c->slot[slot];
    if (!lane_eligible(c, slot, B)) return IRLOSC_OK;
    const size_t waves = ((size_t)c->cfg.max_batch + 63) / 64;
    if (!got(s.blk.ensure(waves * pack_entries() * 64 * sizeof(double))) || !got(s.blk_dq.ensure(qt_bytes(c)))) return IRLOSC_OK;
    PackArgs a;
    memset(&a, 0, sizeof a);
    a.table = c->model.dpack;
    const FeOut<double> rec = slot_out<double>(s);
    a.src[PACK_M] = rec.M; a.src[PACK_J] = rec.J; a.src[PACK_DQ] = rec.dq; a.src[PACK_BIAS] = rec.bias; a.src[PACK_EE] = rec.ee;
    a.blk = s.blk; a.dqb = s.blk_dq;
    a.bad = check ? c->model.dpack_bad : nullptr;
    a.B = B;
    if (check) HIPCHK(c, hipMemsetAsync(a.bad, 0, sizeof(int32_t), c->stream));
    HIPCHK(c, (hipError_t)launch_pack(a, c->stream));
    if (check) {
        int32_t bad = 0;
        HIPCHK(c, hipMemcpyAsync(&bad, a.bad, sizeof bad, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (bad) return IRLOSC_OK;
    }
    s.block_packed(B);
    return IRLOSC_OK;
}

// the eigen pass of the lane form: grid cap, and the flagged robots of a step from which it runs one lane per robot (below: four records
// per wave, row16 form); the choice is made on the device, per step, from the count the lane kernel leaves (A/B measurements)
static int lane_eig_blocks() {
    static const int v = [] { const char* e = getenv("IRLOSC_LANE_EIG_BLOCKS"); const int x = e ? atoi(e) : 0; return x >= 64 && x <= 65536 ? x : 1024; }();
    return v;
}
static int lane_eig_min() {
    static const int v = [] { const char* e = getenv("IRLOSC_LANE_EIG_MIN"); return e ? atoi(e) : 3000; }();
    return v;
}

// Resident lane route: a (sub-)train of n steps on bank k whose slots sl[i] hold a valid compact block -- the lane-per-robot OSC step
// and its eigen pass read the block, the give-up pass (generic kernel) the slot's dense records, which stay valid.  ps[i]: the step's
// parameters with its outputs; pos[i]: the step of the whole train it is (give-up list and counter of that step, as in row16_train).
static int lane_train(irlosc_ctx* c, const KParams<double>* ps, const int* sl, int n, int k, const int* pos, bool first, bool last) {
    if (n < 1 || n > R16_TRAIN) return fail(c, IRLOSC_ERR_STATE, "train of %d steps", n);
    irlosc_ctx::Bank& bk = c->bank[k];
    const hipStream_t st = bk.st;
    if (first) HIPCHK(c, hipMemsetAsync(bk.count, 0, R16_TRAIN * sizeof(int32_t), st));
    c->count_cur = bk.count;
    Row16Train<double> tr;
    memset(&tr, 0, sizeof tr);
    lane::LaneTrain lt;
    memset(&lt, 0, sizeof lt);
    for (int i = 0; i < n; ++i) {
        const int o = pos[i];
        tr.p[i] = ps[i];
        tr.x[i] = Row16Extra{c->dzeros, bk.list[o], bk.count + o, c->slot[sl[i]].blk, nullptr, c->model.dtables, c->span_next, nullptr};
        lt.qt[i] = c->slot[sl[i]].blk_dq;
        lt.rec[i] = bk.lane_rec[i];
        lt.rec_count[i] = bk.lane_count + i;
    }
    lt.map = c->model.lane_map;
    HIPCHK(c, hipMemsetAsync(bk.lane_count, 0, R16_TRAIN * sizeof(int32_t), st));
    if (first && c->tev_begin) HIPCHK(c, hipEventRecord(c->tev_begin, st));
    HIPCHK(c, (hipError_t)launch_lane_osc<double>(tr, lt, n, c->model.lane_tier, lane_eig_blocks(), lane_eig_min(), st));
    if (c->span_next) HIPCHK(c, (hipError_t)launch_span_end(c->span_next, st));      // (irlosc_time_trains: the step ends with its eigen pass)
    HIPCHK(c, (hipError_t)launch_row16_worklist<double>(tr, n, nullptr, st));
    if (last && c->tev_end) HIPCHK(c, hipEventRecord(c->tev_end, st));
    return IRLOSC_OK;
}

// fp64-arithmetic path: one launch for a train of n steps (ps[i] complete with its own outputs), whatever the storage
// type T of the records.  All instances run on the row16 kernel, the truncated pseudo-inverse included; the few it gives
// up on (net of eigen-candidates full, degenerate A) are recomputed by the generic kernel (Jacobi, fp64 arithmetic) from
// the lists it leaves behind.  Bank 0 without task rows (out of memory): that train computes part 1 of the task signal in the
// row16 kernel, same results.
template <typename T>
static int row16_train(irlosc_ctx* c, const KParams<T>* ps, int n, bool tree, hipStream_t st, int k = 0, const int* pos = nullptr,
                       bool first = true, bool last = true) {
    // pos[i] = step of the whole train that sub-train step i is (a train that mixes tree-form and dense slots goes out as two
    // sub-trains): give-up list and counter are those of the ORIGINAL step, and only the first sub-train zeroes the counters, so
    // that irlosc_giveup_counts reports every step of the train at its own index; the timing events bracket the whole train.
    if (n < 1 || n > R16_TRAIN) return fail(c, IRLOSC_ERR_STATE, "train of %d steps", n);
    Row16Train<T> tr;
    memset(&tr, 0, sizeof tr);
    irlosc_ctx::Bank& bk = c->bank[k];
    if (first) HIPCHK(c, hipMemsetAsync(bk.count, 0, R16_TRAIN * sizeof(int32_t), st));
    c->count_cur = bk.count;
    const bool rows = c->task_pass && ensure_bank(c, k, n, NEED_ROWS) == 0;
    for (int i = 0; i < n; ++i) {
        const int o = pos ? pos[i] : i;
        tr.p[i] = ps[i];
        tr.x[i] = Row16Extra{c->dzeros, bk.list[o], bk.count + o, nullptr, nullptr, nullptr, c->span_next, rows ? bk.trows[i] : nullptr};
    }
    if (first && c->tev_begin) HIPCHK(c, hipEventRecord(c->tev_begin, st));
    int rc = launch_row16<T>(tr, n, tree, st);
    if (rc) return fail(c, IRLOSC_ERR_HIP, "row16 kernel launch failed: %s", hipGetErrorString((hipError_t)rc));
    HIPCHK(c, (hipError_t)launch_row16_worklist<T>(tr, n, nullptr, st));
    if (last && c->tev_end) HIPCHK(c, hipEventRecord(c->tev_end, st));
    return IRLOSC_OK;
}

template <typename T>
static int launch_t(irlosc_ctx* c, int B, const StepInputs& in, void* u, uint32_t* flags, hipStream_t st, bool tree) {
    KParams<T> p;
    fill_params<T>(c, p, B, in, u, flags);
    if (c->kernel == IRLOSC_KERNEL_ROW16) return row16_train<T>(c, &p, 1, tree, st);
    HIPCHK(c, (hipError_t)launch_generic<T>(p, B, st));
    return IRLOSC_OK;
}

static int launch(irlosc_ctx* c, int B, const StepInputs& in, void* u, uint32_t* flags, hipStream_t st, bool tree = false) {
    if (B == 0) return IRLOSC_OK;
    if (c->gains_nb == 0) return fail(c, IRLOSC_ERR_STATE, "irlosc_set_gains has not been called");
    if (c->cfg.dtype == IRLOSC_F64) return launch_t<double>(c, B, in, u, flags, st, tree);
    return launch_t<float>(c, B, in, u, flags, st, tree);
}

// A step over B instances needs B instances of state AND of targets in the slot (stale or uninitialised HBM otherwise).
static int check_slot_filled(irlosc_ctx* c, int slot, int B) {
    const Slot& s = c->slot[slot];
    if (!s.records && s.fused_away)
        return fail(c, IRLOSC_ERR_STATE, "slot %d holds no dense records: the preceding fused irlosc_step_from_q / irlosc_step_resident_from_q "
                    "invalidated them (it never writes M / J); run irlosc_frontend or an upload first", slot);
    if (!s.records || !s.targets)
        return fail(c, IRLOSC_ERR_STATE, "slot %d: irlosc_upload and irlosc_set_targets must precede a step", slot);
    if (B > std::max(0, s.records) || B > std::max(0, s.targets))
        return fail(c, IRLOSC_ERR_STATE, "slot %d holds state for %d and targets for %d instances, step asked for %d", slot,
                    std::max(0, s.records), std::max(0, s.targets), B);
    return IRLOSC_OK;
}

// feed_wr: the wrench computed from the slot's sensor feed (a step from joint coordinates), else the record wrench of the last upload
static int launch_slot(irlosc_ctx* c, int slot, int B, const void* feed_wr = nullptr) {
    int rcf = check_slot_filled(c, slot, B);
    if (rcf) return rcf;
    const int route = record_route(c, slot, B);
    if (route == IRLOSC_ROUTE_LANE && c->gains_nb > 0 && !feed_wr) {      // the resident lane route, as irlosc_step_resident takes it
        if (ensure_bank(c, 0, 1, NEED_LANE) == 0) {
            KParams<double> p;
            fill_params<double>(c, p, B, slot_inputs(c->slot[slot]), c->du, c->dflags);
            const int pos = 0;
            return lane_train(c, &p, &slot, 1, 0, &pos, true, true);
        }
        free_bank(c->bank[0], NEED_LANE);
    }
    return launch(c, B, slot_inputs(c->slot[slot], feed_wr), c->du, c->dflags, c->stream, row16_route(route) == IRLOSC_ROUTE_ROW16_TREE);
}

extern "C" int irlosc_download(irlosc_ctx* c, int32_t B, void* u_host, uint32_t* flags_host) {
    if (!c) return IRLOSC_ERR_ARG;
    if (B < 0 || B > c->cfg.max_batch) return fail(c, IRLOSC_ERR_ARG, "B out of range");
    HIPCHK(c, hipSetDevice(c->cfg.hip_device));
    if (u_host && B) HIPCHK(c, hipMemcpyAsync(u_host, c->du, (size_t)B * c->cfg.n * c->esz, hipMemcpyDeviceToHost, c->stream));
    if (flags_host && B) HIPCHK(c, hipMemcpyAsync(flags_host, c->dflags, (size_t)B * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->ddbg && B >= 16) {   // debug: mean cycles per phase over all waves
        const bool r16 = c->kernel == IRLOSC_KERNEL_ROW16;
        const bool lanef = getenv("IRLOSC_PHASE_LANE") != nullptr;      // a -DIRLOSC_LANE_STAMPS build: the lane kernel of the fused path stamped
        const int tiles = lanef ? B / 64 : r16 ? B / 4 : B / 16;
        std::vector<unsigned long long> h((size_t)tiles * 10);
        HIPCHK(c, hipMemcpy(h.data(), c->ddbg, h.size() * 8, hipMemcpyDeviceToHost));
        static const char* nm_g[7] = {"vec-wait", "M-stream+Cholesky", "J+fwd-subst", "task-error", "A=YtY", "kxk", "torques+store"};
        static const char* nm_r[7] = {"loads+task-error", "J->LDS", "main-loop", "A=YtY", "kxk", "eigen", "torques+store"};
        static const char* nm_l[7] = {"first-requests+task-rows", "recursion", "kxk", "records", "Jt+sums", "torques+store", "-"};
        const char* const* nm = lanef ? nm_l : r16 ? nm_r : nm_g;
        double acc[7] = {0}, rt = 0;
        unsigned long long rmin = ~0ull, rmax = 0;
        for (int t = 0; t < tiles; ++t) {
            for (int i = 0; i < 7; ++i) acc[i] += (double)(h[(size_t)t * 10 + i + 1] - h[(size_t)t * 10 + i]);
            const unsigned long long r0 = h[(size_t)t * 10 + 8] & 0x0fffffffffffffffull;
            rt += (double)(h[(size_t)t * 10 + 9] - r0);
            rmin = std::min(rmin, r0);
            rmax = std::max(rmax, h[(size_t)t * 10 + 9]);
        }
        if (!r16) {   // where do blocks land?  XCC of tile t vs t % 8, and vs the XCC of tile t + 2048; start order of the second round
            int same_mod = 0, same_next = 0, cnt_next = 0;
            for (int t = 0; t < tiles; ++t) {
                const int x = (int)(h[(size_t)t * 10 + 8] >> 60);
                same_mod += (x == (t % 8));
                if (t + 2048 < tiles) { ++cnt_next; same_next += (x == (int)(h[(size_t)(t + 2048) * 10 + 8] >> 60)); }
            }
            fprintf(stderr, "[irlosc placement] xcc==tile%%8: %d/%d, xcc(t)==xcc(t+2048): %d/%d; xcc of tiles 0..15:", same_mod, tiles, same_next, cnt_next);
            for (int t = 0; t < 16 && t < tiles; ++t) fprintf(stderr, " %d", (int)(h[(size_t)t * 10 + 8] >> 60));
            fprintf(stderr, "\n");
        }
        double tot = 0; for (int i = 0; i < 7; ++i) tot += acc[i];
        fprintf(stderr, "[irlosc phase timing] %d waves, mean cycles/wave %.0f:", tiles, tot / tiles);
        for (int i = 0; i < 7; ++i) fprintf(stderr, " %s=%.0f", nm[i], acc[i] / tiles);
        // s_memrealtime ticks at 100 MHz: wave residency in us, the shader clock it implies, first start -> last end
        fprintf(stderr, " | wave %.2f us => %.0f MHz, launch span %.2f us\n", rt / tiles / 100.0,
                (tot / tiles) / (rt / tiles / 100.0), (double)(rmax - rmin) / 100.0);
    }
    return IRLOSC_OK;
}

extern "C" int irlosc_step(irlosc_ctx* c, int32_t slot, int32_t B, void* u_host, uint32_t* flags_host) {
    if (!c) return IRLOSC_ERR_ARG;
    int rc = check_slot(c, slot, B);
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->cfg.hip_device));
    rc = launch_slot(c, slot, B);
    if (rc) return rc;
    if (u_host || flags_host) return irlosc_download(c, B, u_host, flags_host);
    return IRLOSC_OK;
}

// A train of n steps on bank k: step i runs slot slots[i] and writes the bank's output set i.
typedef int (*TrainFn)(irlosc_ctx* c, const int* slots, int n, int B, int k);

// `iters` steps as trains of at most R16_TRAIN steps, train t on bank t % nbanks (irlosc_ctx::Bank); banks that cannot be allocated are
// done without, and with timing events attached every train runs on the main stream.  The other banks' streams start behind whatever the
// main stream holds, and the main stream continues behind all of them -- on every exit, so that trains enqueued before an error stay
// ordered before later work on it.
static int run_trains(irlosc_ctx* c, int first_slot, int B, int iters, int nbanks, unsigned need, TrainFn train) {
    int nb = 1;
    while (!c->tev_begin && nb < nbanks && ensure_bank(c, nb, R16_TRAIN, need) == 0) ++nb;
    if (nb > 1) HIPCHK(c, hipEventRecord(c->ev_join, c->stream));
    for (int k = 1; k < nb; ++k) HIPCHK(c, hipStreamWaitEvent(c->bank[k].st, c->ev_join, 0));
    int rc = IRLOSC_OK;
    for (int done = 0, t = 0; done < iters && !rc; done += R16_TRAIN, ++t) {
        const int n = std::min((int)R16_TRAIN, iters - done), k = t % nb;
        int slots[R16_TRAIN];
        for (int i = 0; i < n; ++i) slots[i] = (first_slot + done + i) % c->cfg.n_slots;
        rc = train(c, slots, n, B, k);
        if (!rc) { c->du = c->bank[k].u[n - 1]; c->dflags = c->bank[k].flags[n - 1]; c->count_cur = c->bank[k].count; }
    }
    for (int k = 1; k < nb; ++k) {
        hipError_t e = hipEventRecord(c->bank[k].done, c->bank[k].st);
        if (e == hipSuccess) e = hipStreamWaitEvent(c->stream, c->bank[k].done, 0);
        if (e != hipSuccess && !rc) rc = fail(c, IRLOSC_ERR_HIP, "joining the stream of bank %d failed: %s", k, hipGetErrorString(e));
    }
    return rc;
}

// A train on dense records.  One kernel per launch, so a train whose slots do not ALL qualify for the tree-structured form is issued as
// two sub-trains -- the qualifying steps with the tree kernel, the others with the dense recursion -- instead of dropping every step to
// the dense recursion (one more launch, only when slots are mixed).
// Slots of the resident lane route go out as a third sub-train, ahead of the other two (lane_train).
template <typename T>
static int dense_train(irlosc_ctx* c, const int* slots, int n, int B, int k) {
    irlosc_ctx::Bank& bk = c->bank[k];
    constexpr int R0 = IRLOSC_ROUTE_ROW16, NR = IRLOSC_ROUTE_LANE - R0 + 1;      // sub-trains by record_route: dense, tree form, lane
    KParams<T> ps[NR][R16_TRAIN];
    int pos[NR][R16_TRAIN];             // step of the train each sub-train step is
    int sl[NR][R16_TRAIN];              // its slot
    int cnt[NR] = {};
    bool lane_ok = false;               // some slot takes the route: the bank's lane records (out of memory: the row16 kernel)
    for (int i = 0; i < n; ++i) lane_ok = lane_ok || record_route(c, slots[i], B) == IRLOSC_ROUTE_LANE;
    if (lane_ok && ensure_bank(c, k, n, NEED_LANE)) { free_bank(bk, NEED_LANE); lane_ok = false; }
    for (int i = 0; i < n; ++i) {
        const int slot = slots[i];
        int rcf = check_slot_filled(c, slot, B);
        if (rcf) return rcf;
        const int route = record_route(c, slot, B), r = (lane_ok ? route : row16_route(route)) - R0;
        pos[r][cnt[r]] = i;
        sl[r][cnt[r]] = slot;
        fill_params<T>(c, ps[r][cnt[r]++], B, slot_inputs(c->slot[slot]), bk.u[i], bk.flags[i]);
    }
    int first = -1, last = -1;      // order: lane sub-train, tree sub-train, dense sub-train
    for (int r = NR - 1; r >= 0; --r) if (cnt[r]) { if (first < 0) first = r; last = r; }
    for (int r = NR - 1; r >= 0; --r) {
        if (!cnt[r]) continue;
        int rc;
        if constexpr (std::is_same<T, double>::value)      // (the lane route: float64 records only, lane_eligible)
            rc = r + R0 == IRLOSC_ROUTE_LANE ? lane_train(c, ps[r], sl[r], cnt[r], k, pos[r], r == first, r == last)
                                             : row16_train<T>(c, ps[r], cnt[r], r + R0 == IRLOSC_ROUTE_ROW16_TREE, bk.st, k, pos[r], r == first, r == last);
        else
            rc = row16_train<T>(c, ps[r], cnt[r], r + R0 == IRLOSC_ROUTE_ROW16_TREE, bk.st, k, pos[r], r == first, r == last);
        if (rc) return rc;
    }
    return IRLOSC_OK;
}

// `iters` steps on the row16 path from dense records.  More than one train: odd trains on the second bank (a call of exactly one full
// train already allocates it: a caller's warm-up then pays for it, not its timed loop).
static int row16_resident(irlosc_ctx* c, int first_slot, int B, int iters) {
    bool lane = false;
    for (int i = 0; i < std::min(iters, c->cfg.n_slots) && !lane; ++i) lane = record_route(c, (first_slot + i) % c->cfg.n_slots, B) == IRLOSC_ROUTE_LANE;
    return run_trains(c, first_slot, B, iters, c->r16_overlap && iters >= R16_TRAIN ? irlosc_ctx::R16_BANKS : 1,
                      (c->task_pass ? NEED_ROWS : 0) | (lane ? NEED_LANE : 0), c->cfg.dtype == IRLOSC_F64 ? dense_train<double> : dense_train<float>);
}

// The shared frame of irlosc_step_resident and irlosc_step_resident_from_q: the argument checks, `steps()` (the `iters` steps, enqueued)
// between the context's event pair, and the time of the whole and per step.
template <typename Steps>
static int timed_resident(irlosc_ctx* c, int first_slot, int B, int iters, float* ms_total, float* ms_avg, Steps steps) {
    if (!c) return IRLOSC_ERR_ARG;
    int rc = check_slot(c, first_slot, B);
    if (rc) return rc;
    if (iters < 1) return fail(c, IRLOSC_ERR_ARG, "iters must be >= 1");
    if (c->gains_nb == 0) return fail(c, IRLOSC_ERR_STATE, "irlosc_set_gains has not been called");
    HIPCHK(c, hipSetDevice(c->cfg.hip_device));
    HIPCHK(c, hipEventRecord(c->ev0, c->stream));
    rc = steps();
    if (rc) return rc;
    HIPCHK(c, hipEventRecord(c->ev1, c->stream));
    HIPCHK(c, hipEventSynchronize(c->ev1));
    float ms = 0.f;
    HIPCHK(c, hipEventElapsedTime(&ms, c->ev0, c->ev1));
    if (ms_total) *ms_total = ms;
    if (ms_avg) *ms_avg = ms / (float)iters;
    return IRLOSC_OK;
}

extern "C" int irlosc_step_resident(irlosc_ctx* c, int32_t first_slot, int32_t B, int32_t iters, float* ms_total,
                                    float* ms_kernel_avg) {
    return timed_resident(c, first_slot, B, iters, ms_total, ms_kernel_avg, [&] {
        if (c->kernel == IRLOSC_KERNEL_ROW16 && B > 0) return row16_resident(c, first_slot, B, iters);
        int rc = IRLOSC_OK;
        for (int i = 0; i < iters && !rc; ++i) rc = launch_slot(c, (first_slot + i) % c->cfg.n_slots, B);
        return rc;
    });
}

extern "C" int irlosc_steps_per_launch(const irlosc_ctx* c) {
    if (!c) return IRLOSC_ERR_ARG;
    return c->kernel == IRLOSC_KERNEL_GENERIC ? 1 : c->train;
}

static int fused_resident(irlosc_ctx* c, int first_slot, int B, int iters);
static bool fused_ready(irlosc_ctx* c, int n);

// One untimed train first (clocks, caches: nothing rides on an idle machine), then `ntrains` one-train calls back to back on the main
// stream, train i bracketed by the event pair tev_pool[2 i], [2 i + 1] (and, with `spans`, stamped by its kernels at dspan + i).  Train j
// of the sequence starts at slot first_slot + j * train.
static int timed_trains(irlosc_ctx* c, int first_slot, int B, int ntrains, bool from_q, bool spans) {
    while ((int)c->tev_pool.size() < 2 * ntrains) {
        Event ev;
        HIPCHK(c, ev.ensure());
        c->tev_pool.push_back(std::move(ev));
    }
    int rc = IRLOSC_OK;
    for (int i = -1; i < ntrains && !rc; ++i) {
        if (i >= 0) {
            c->tev_begin = c->tev_pool[2 * i]; c->tev_end = c->tev_pool[2 * i + 1];
            if (spans) c->span_next = c->dspan + (size_t)R16_SPAN_WORDS * i;
        }
        const int s0 = (first_slot + (i + 1) * c->train) % c->cfg.n_slots;
        rc = from_q ? fused_resident(c, s0, B, c->train) : row16_resident(c, s0, B, c->train);
        c->tev_begin = c->tev_end = nullptr;
        c->span_next = nullptr;
    }
    return rc;
}

extern "C" int irlosc_time_dominant_kernel(irlosc_ctx* c, int32_t slot, int32_t B, int32_t iters, float* ms_avg) {
    if (!c) return IRLOSC_ERR_ARG;
    int rc = check_slot(c, slot, B);
    if (rc) return rc;
    if (iters < 1 || iters > 256 || !ms_avg) return fail(c, IRLOSC_ERR_ARG, "iters must be in [1,256] and ms_avg non-NULL");
    HIPCHK(c, hipSetDevice(c->cfg.hip_device));
    if (c->kernel == IRLOSC_KERNEL_GENERIC || B == 0) {        // generic path: a step IS the dominant kernel
        float tot = 0.f;
        rc = irlosc_step_resident(c, slot, B, iters, &tot, ms_avg);
        return rc;
    }
    // row16 path: the same trains as irlosc_step_resident, on one stream, with a HIP event pair around each (task pass + row16 kernel +
    // give-up pass) -- what a rocprofv3 kernel trace of the timed region shows, so the two averages are comparable.
    if (c->gains_nb == 0) return fail(c, IRLOSC_ERR_STATE, "irlosc_set_gains has not been called");
    const int launches = std::max(1, iters / c->train);
    rc = timed_trains(c, slot, B, launches, false, false);
    if (rc) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    double tot = 0.0;
    for (int i = 0; i < launches; ++i) {
        float ms = 0.f;
        HIPCHK(c, hipEventElapsedTime(&ms, c->tev_pool[2 * i], c->tev_pool[2 * i + 1]));
        tot += ms;
    }
    *ms_avg = (float)(tot / launches);
    return IRLOSC_OK;
}

// Roofline evidence without a tracer (include/irlosc.h): per train one HIP event pair AND the wall-clock stamps the train's
// main kernel takes itself (first wave's start, last wave's end).
extern "C" int irlosc_time_trains(irlosc_ctx* c, int32_t first_slot, int32_t B, int32_t ntrains, int32_t from_q, double* out) {
    if (!c) return IRLOSC_ERR_ARG;
    int rc = check_slot(c, first_slot, B);
    if (rc) return rc;
    if (ntrains < 1 || ntrains > 4096 || !out) return fail(c, IRLOSC_ERR_ARG, "ntrains must be in [1,4096] and out non-NULL");
    if (c->kernel != IRLOSC_KERNEL_ROW16 || B < 1) return fail(c, IRLOSC_ERR_ARG, "irlosc_time_trains needs the row16 kernel and B >= 1");
    if (c->gains_nb == 0) return fail(c, IRLOSC_ERR_STATE, "irlosc_set_gains has not been called");
    HIPCHK(c, hipSetDevice(c->cfg.hip_device));
    if (from_q && !fused_ready(c, c->train)) return fail(c, IRLOSC_ERR_STATE, "the fused path from joint coordinates is not available on this context");
    HIPCHK(c, c->dspan.reserve((size_t)ntrains * R16_SPAN_WORDS * sizeof(unsigned long long)));
    std::vector<unsigned long long> h((size_t)ntrains * R16_SPAN_WORDS);
    for (int i = 0; i < ntrains; ++i) {
        unsigned long long* t = h.data() + (size_t)i * R16_SPAN_WORDS;
        for (int s2 = 0; s2 < R16_SPAN_SLOTS; ++s2) { t[2 * s2] = ~0ull; t[2 * s2 + 1] = 0ull; }
        t[2 * R16_SPAN_SLOTS] = t[2 * R16_SPAN_SLOTS + 1] = 0ull;
    }
    HIPCHK(c, hipMemcpyAsync(c->dspan, h.data(), h.size() * sizeof(unsigned long long), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    rc = timed_trains(c, first_slot, B, ntrains, from_q, true);
    if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(h.data(), c->dspan, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    unsigned long long t0 = 0;
    for (int i = 0; i < ntrains; ++i) {
        unsigned long long lo = ~0ull, hi = 0ull;                    // over the stamp pairs of the train
        const unsigned long long* t = h.data() + (size_t)i * R16_SPAN_WORDS;
        for (int s2 = 0; s2 < R16_SPAN_SLOTS; ++s2) {
            lo = std::min(lo, t[2 * s2]);
            hi = std::max(hi, t[2 * s2 + 1]);
        }
        if (i == 0) t0 = lo;
        float ms = 0.f;
        HIPCHK(c, hipEventElapsedTime(&ms, c->tev_pool[2 * i], c->tev_pool[2 * i + 1]));
        out[4 * i] = ms;
        out[4 * i + 1] = (double)(lo - t0) / 100.0;                  // s_memrealtime: 100 MHz
        out[4 * i + 2] = (double)(hi - t0) / 100.0;
        out[4 * i + 3] = t[2 * R16_SPAN_SLOTS + 1] ? (double)t[2 * R16_SPAN_SLOTS] / ((double)t[2 * R16_SPAN_SLOTS + 1] / 100.0) : 0.0;   // cycles per us = MHz
    }
    return IRLOSC_OK;
}

// Instances the most recent step / train handed from the row16 kernel's in-wave eigen stage to the generic kernel (the give-up
// lists): counters of the last train, read back after a stream synchronisation.
extern "C" int irlosc_giveup_counts(irlosc_ctx* c, int32_t* out) {
    if (!c || !out) return IRLOSC_ERR_ARG;
    for (int i = 0; i < R16_TRAIN; ++i) out[i] = 0;
    if (c->kernel != IRLOSC_KERNEL_ROW16) return IRLOSC_OK;
    HIPCHK(c, hipSetDevice(c->cfg.hip_device));
    HIPCHK(c, hipMemcpyAsync(out, c->count_cur, R16_TRAIN * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return IRLOSC_OK;
}

extern "C" int irlosc_sync(irlosc_ctx* c) {
    if (!c) return IRLOSC_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->cfg.hip_device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return IRLOSC_OK;
}

// ---- rigid-body front end ------------------------------------------------------------------------------------------
// q (w x y z) -> row-major rotation; `normalise`: of q / |q| (a caller's quaternion), else q is taken as given (the model's own, as the
// kernels take them)
static void quat_mat(const double* q, double* R, bool normalise) {
    const double nq = normalise ? std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]) : 1.0;      // (x / 1.0 is x, bit for bit)
    const double w = q[0] / nq, x = q[1] / nq, y = q[2] / nq, z = q[3] / nq;
    R[0] = 1 - 2 * (y * y + z * z); R[1] = 2 * (x * y - w * z); R[2] = 2 * (x * z + w * y);
    R[3] = 2 * (x * y + w * z); R[4] = 1 - 2 * (x * x + z * z); R[5] = 2 * (y * z - w * x);
    R[6] = 2 * (x * z - w * y); R[7] = 2 * (y * z + w * x); R[8] = 1 - 2 * (x * x + y * y);
}

// Validate and derive: the caller's model checked against the cfg and turned into the walk's tables.  A pure function of `m`, c->cfg and
// c->k (of the context it writes the error text only); every IRLOSC_ERR_ARG of irlosc_set_model is returned here.
static int derive_model(irlosc_ctx* c, const irlosc_model* m, FeModel& h) {
    if (!m) return fail(c, IRLOSC_ERR_ARG, "model is NULL");
    if (m->nb < 1 || m->nb > IRLOSC_MAX_BODIES) return fail(c, IRLOSC_ERR_ARG, "nb=%d out of [1,%d]", m->nb, IRLOSC_MAX_BODIES);
    if (m->nj != c->cfg.n) return fail(c, IRLOSC_ERR_ARG, "model has %d hinges but cfg.n = %d", m->nj, c->cfg.n);
    memset(&h, 0, sizeof h);
    h.nb = m->nb; h.nj = m->nj; h.ndev = c->cfg.ndev; h.k = c->k;
    std::vector<int> seen(m->nj, 0);
    for (int b = 0; b < m->nb; ++b) {
        const int par = m->parent[b], jb = m->joint_of_body[b];
        if (par >= b || par < -1) return fail(c, IRLOSC_ERR_ARG, "body %d: parent %d must precede it (or be -1)", b, par);
        if (jb < -1 || jb >= m->nj) return fail(c, IRLOSC_ERR_ARG, "body %d: hinge index %d out of range", b, jb);
        if (jb >= 0 && seen[jb]++) return fail(c, IRLOSC_ERR_ARG, "hinge %d sits on two bodies", jb);
        if (!(m->mass[b] >= 0.0)) return fail(c, IRLOSC_ERR_ARG, "body %d: negative mass", b);
        h.parent[b] = par; h.joint_of_body[b] = jb;
        h.depth[b] = par < 0 ? 0 : h.depth[par] + 1;
        h.maxdepth = std::max(h.maxdepth, h.depth[b]);
        h.anc_mask[b] = (par < 0 ? 0u : h.anc_mask[par]) | (jb >= 0 ? 1u << jb : 0u);
        if (jb >= 0) h.body_of_joint[jb] = b;
        for (int i = 0; i < 3; ++i) { h.pos[b][i] = m->pos[b][i]; h.ipos[b][i] = m->ipos[b][i]; h.inertia[b][i] = m->inertia[b][i]; }
        for (int i = 0; i < 4; ++i) { h.quat[b][i] = m->quat[b][i]; h.iquat[b][i] = m->iquat[b][i]; }
        h.mass[b] = m->mass[b];
    }
    for (int j = 0; j < m->nj; ++j) {
        if (!seen[j]) return fail(c, IRLOSC_ERR_ARG, "hinge %d sits on no body", j);
        for (int i = 0; i < 3; ++i) { h.jaxis[j][i] = m->jaxis[j][i]; h.jpos[j][i] = m->jpos[j][i]; }
        h.armature[j] = m->armature[j];
        for (int b = 0; b < m->nb; ++b) if ((h.anc_mask[b] >> j) & 1u) h.sub_mask[j] |= 1ull << b;
    }
    for (int i = 0; i < 3; ++i) h.gravity[i] = m->gravity[i];
    for (int b = 0; b < m->nb; ++b) {      // derived tables of the lane-per-instance kernel
        double R[9];
        const int jb = h.joint_of_body[b];
        if (jb >= 0) {
            quat_mat(h.quat[b], R, false);
            for (int r = 0; r < 3; ++r) h.jpos_par[jb][r] = R[r * 3] * h.jpos[jb][0] + R[r * 3 + 1] * h.jpos[jb][1] + R[r * 3 + 2] * h.jpos[jb][2];
        }
        for (int j = 0; j < m->nj; ++j) if ((h.anc_mask[b] >> j) & 1u) h.cmass[j] += h.mass[b];
        quat_mat(h.iquat[b], R, false);
        int e = 0;
        for (int r = 0; r < 3; ++r)
            for (int cc = r; cc < 3; ++cc)
                h.icb[b][e++] = R[r * 3] * h.inertia[b][0] * R[cc * 3] + R[r * 3 + 1] * h.inertia[b][1] * R[cc * 3 + 1] + R[r * 3 + 2] * h.inertia[b][2] * R[cc * 3 + 2];
    }
    for (int b = 0; b < m->nb; ++b) {      // the per-body records of the walk (FeModel::rec)
        double* w = h.rec[b];
        const int jb = h.joint_of_body[b];
        for (int i = 0; i < 3; ++i) { w[i] = h.pos[b][i]; w[7 + i] = h.ipos[b][i]; }
        for (int i = 0; i < 4; ++i) w[3 + i] = h.quat[b][i];
        for (int i = 0; i < 6; ++i) w[10 + i] = h.icb[b][i];
        w[16] = h.mass[b];
        for (int i = 0; i < 3; ++i) { w[17 + i] = jb >= 0 ? h.jaxis[jb][i] : 0.0; w[20 + i] = jb >= 0 ? h.jpos[jb][i] : 0.0; w[23 + i] = jb >= 0 ? h.jpos_par[jb][i] : 0.0; }
    }
    int row = 0;
    for (int d = 0; d < c->cfg.ndev; ++d) {
        if (m->ee_body[d] < 0 || m->ee_body[d] >= m->nb) return fail(c, IRLOSC_ERR_ARG, "ee_body[%d]=%d out of range", d, m->ee_body[d]);
        h.ee_body[d] = m->ee_body[d];
        h.row0[d] = row; row += c->cfg.dev_rows[d];
        for (int i = 0; i < 6; ++i) if (c->cfg.ctrlr_dof[d][i]) h.dofmask[d] |= 1u << i;
    }
    return IRLOSC_OK;
}

// Plan the routes of the derived model `h` on this context: which front end, whether the fused path, which OSC step behind its walk,
// whether the resident lane route -- with the tables each needs.  Host arithmetic and the A/B switches of the environment only.
void ModelPlan::plan_routes(const irlosc_ctx* c) {
    fe_smem = frontend_smem_bytes(h.nb, h.nj);
    // IRLOSC_FRONTEND=generic: force the wave-per-instance kernel (A/B measurements); IRLOSC_WALK=general: the shape-only walk on the
    // fused path (A/B measurements, tests)
    fe_lane = frontend_lane_dual_ur5_matches(h) && !env_is("IRLOSC_FRONTEND", "generic");
    fe_lane_s = fe_lane && frontend_lane_dual_ur5_s_matches(h) && !env_is("IRLOSC_WALK", "general");
    // The fused path needs the compiled tree shape (lane kernel) and the fp64 row16 kernel; IRLOSC_FUSED=0 forces the
    // two-kernel path through dense records (A/B measurements).
    fused = fe_lane && c->kernel == IRLOSC_KERNEL_ROW16 && !env_off("IRLOSC_FUSED");
    fq_overlap = !env_off("IRLOSC_FQ_OVERLAP");      // "0": consecutive fused trains on one stream (A/B measurements, tests)
    if (!fused) return;
    frontend_lane_dual_ur5_tables(h, &tables);
    fe_xentries = tables.n_entries;
    for (int d = 0; d < c->cfg.ndev; ++d) ft_qe[d] = tables.eetab[d][3];
    // The OSC step behind the walk: lane-per-robot form when an instantiation holds this layout (IRLOSC_LANE=0: the row16 FROMQ
    // kernel, A/B measurements and tests) -- and then the resident lane route, when the layout has a pack table
    lane_tier = env_off("IRLOSC_LANE") ? -1 : lane_plan(h, &lane_map);
    pack_ok = lane_tier >= 0 && pack_plan(h, &pack);
}

// The plan becomes the context's model.  No model is in force from the first line to the last: a HIP failure in between leaves the
// context as it was before its first irlosc_set_model (the entry points from joint coordinates answer IRLOSC_ERR_STATE, no slot takes
// the lane route), not between two models.  `p` outlives the call: one synchronisation behind all uploads -- with which no train of
// any bank is in flight either, so the banks can be freed.
int Model::commit(irlosc_ctx* c, const ModelPlan& p) {
    // Every bank's exchange buffers and lane records start over with another entry count or layout (they are allocated again by the
    // first fused train: ensure_bank)
    const bool resize = p.fused && (p.fe_xentries != fe_xentries || p.lane_tier != lane_tier ||
                                    (p.lane_tier >= 0 && memcmp(&p.lane_map, &lane_map, sizeof lane_map)));
    in_force = 0;
    static_cast<ModelPlan&>(*this) = ModelPlan{};
    HIPCHK(c, dmodel.ensure(sizeof(FeModel)));
    if (p.fused) HIPCHK(c, dtables.ensure(sizeof(FeCompactTables)));
    if (p.pack_ok) HIPCHK(c, dpack.ensure(sizeof(PackTable)));
    if (p.pack_ok) HIPCHK(c, dpack_bad.ensure(sizeof(int32_t)));
    // (the lane front end's side buffer -- 139 MB at 65 536 robots -- is allocated by the first irlosc_frontend: a context that only
    // ever takes the fused path never needs it)
    for (Slot& s : c->slot) {      // the first model of the context: the slots' coordinate buffers
        HIPCHK(c, s.qpos.ensure((size_t)c->cfg.max_batch * c->cfg.n * sizeof(double)));
        HIPCHK(c, s.qvel.ensure((size_t)c->cfg.max_batch * c->cfg.n * sizeof(double)));
    }
    HIPCHK(c, hipMemcpyAsync(dmodel, &p.h, sizeof p.h, hipMemcpyHostToDevice, c->stream));
    if (p.fused) HIPCHK(c, hipMemcpyAsync(dtables, &p.tables, sizeof p.tables, hipMemcpyHostToDevice, c->stream));
    if (p.pack_ok) HIPCHK(c, hipMemcpyAsync(dpack, &p.pack, sizeof p.pack, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    static_cast<ModelPlan&>(*this) = p;
    // what was laid out for the old model: bank buffers, every slot's compact block (built again by its next upload / front end) and
    // sensor feed, the F/T description (site bodies, R_rel)
    if (resize) for (irlosc_ctx::Bank& bk : c->bank) free_bank(bk, NEED_X | NEED_LANE);
    for (Slot& s : c->slot) s.model_changed();
    c->ft_set = 0;
    c->plant_set = 0;      // (its joint mask was checked against another model's hinges)
    if (fused) {      // coordinates uploaded while the fused path was off: laid out for the walk here, not by a train on another stream
        for (Slot& s : c->slot) {
            if (s.coords <= 0) continue;
            HIPCHK(c, s.qt.ensure(qt_bytes(c)));
            HIPCHK(c, (hipError_t)launch_q_layout(s.qpos, s.qvel, s.qt, s.coords, c->cfg.n, c->stream));
        }
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    in_force = 1;
    return IRLOSC_OK;
}

extern "C" int irlosc_set_model(irlosc_ctx* c, const irlosc_model* m) {
    if (!c) return IRLOSC_ERR_ARG;
    ModelPlan p;
    const int rc = derive_model(c, m, p.h);      // refused: the model in force stays, whole
    if (rc) return rc;
    p.plan_routes(c);
    HIPCHK(c, hipSetDevice(c->cfg.hip_device));
    return c->model.commit(c, p);
}

extern "C" int irlosc_upload_q(irlosc_ctx* c, int32_t slot, int32_t B, const double* qpos, const double* qvel) {
    if (!c) return IRLOSC_ERR_ARG;
    int rc = check_slot(c, slot, B);
    if (rc) return rc;
    if (!c->model.in_force) return fail(c, IRLOSC_ERR_STATE, "irlosc_set_model has not been called");
    Slot& s = c->slot[slot];
    if (B == 0) { s.coords = -1; return IRLOSC_OK; }
    if (!qpos || !qvel) return fail(c, IRLOSC_ERR_ARG, "qpos and qvel are required");
    HIPCHK(c, hipSetDevice(c->cfg.hip_device));
    const size_t bytes = (size_t)B * c->cfg.n * sizeof(double);
    HIPCHK(c, hipMemcpyAsync(s.qpos, qpos, bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(s.qvel, qvel, bytes, hipMemcpyHostToDevice, c->stream));
    // the fused walk reads its own layout of the same numbers ([wave][2 n][64 robots]: coalesced, hinge by hinge): one small kernel
    // behind the copies (10 us per 65 536 robots against 0.8 ms of PCIe for them)
    // (only the fused path reads this layout; its buffer is allocated by the slot's first upload while the path is on, or by the
    //  irlosc_set_model that turns it on -- and, once it exists, refreshed by EVERY upload: a copy left stale while another model had
    //  the path switched off would be walked later)
    if (c->model.fused) HIPCHK(c, s.qt.ensure(qt_bytes(c)));
    if (s.qt) HIPCHK(c, (hipError_t)launch_q_layout(s.qpos, s.qvel, s.qt, B, c->cfg.n, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    s.coords = B;
    return IRLOSC_OK;
}

// qpos / qvel: the caller's device arrays instead of the slot's coordinates, on stream `cst` (irlosc_step_from_q_device)
static int frontend_launch(irlosc_ctx* c, int slot, int B, const double* qpos = nullptr, const double* qvel = nullptr, hipStream_t cst = nullptr) {
    if (!c->model.in_force) return fail(c, IRLOSC_ERR_STATE, "irlosc_set_model has not been called");
    Slot& s = c->slot[slot];
    if (!qpos && !s.coords) return fail(c, IRLOSC_ERR_STATE, "slot %d: irlosc_upload_q must precede irlosc_frontend", slot);
    s.drop_block(false);
    if (B == 0) { s.emptied(); return IRLOSC_OK; }
    if (!qpos && B > s.coords) return fail(c, IRLOSC_ERR_STATE, "slot %d holds joint coordinates of %d instances, front end asked for %d", slot, std::max(0, s.coords), B);
    if (!qpos) { qpos = s.qpos; qvel = s.qvel; }
    const hipStream_t st = cst ? cst : c->stream;
    Model& m = c->model;
    if (m.fe_lane && !got(m.fe_side.ensure((((size_t)c->cfg.max_batch + 63) / 64) * frontend_lane_dual_ur5_side_doubles_per_wave() * sizeof(double))))
        m.give_up_lane_walk();
    s.writing();
    int rc;
    if (c->cfg.dtype == IRLOSC_F64) {
        const FeOut<double> o = slot_out<double>(s);
        rc = m.fe_lane ? launch_frontend_lane_dual_ur5<double>(m.dmodel, qpos, qvel, o, B, m.fe_side, st)
                       : launch_frontend_generic<double>(m.dmodel, qpos, qvel, o, B, m.fe_smem, st);
    } else {
        const FeOut<float> o = slot_out<float>(s);
        rc = m.fe_lane ? launch_frontend_lane_dual_ur5<float>(m.dmodel, qpos, qvel, o, B, m.fe_side, st)
                       : launch_frontend_generic<float>(m.dmodel, qpos, qvel, o, B, m.fe_smem, st);
    }
    HIPCHK(c, (hipError_t)rc);
    // The records of this slot are now those of B robots: an earlier, larger upload must not vouch for instances the front
    // end did not write (the wrench of the slot stays what the last irlosc_upload / irlosc_upload_raw put there).
    s.accepted(B, s.has_wrench, m.fe_lane);     // the lane kernel walks the compiled tree: its records carry the tree's zeros by construction
    // (and so need no check for the compact block of the lane route; a caller's stream gets no pack: the slot steps on the row16 kernel)
    return cst ? IRLOSC_OK : pack_slot(c, slot, B, false);
}

extern "C" int irlosc_frontend(irlosc_ctx* c, int32_t slot, int32_t B) {
    if (!c) return IRLOSC_ERR_ARG;
    int rc = check_slot(c, slot, B);
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->cfg.hip_device));
    return frontend_launch(c, slot, B);
}

extern "C" int irlosc_download_records(irlosc_ctx* c, int32_t slot, int32_t B, void* M, void* J, void* dq, void* bias,
                                       void* ee_pose) {
    if (!c) return IRLOSC_ERR_ARG;
    int rc = check_slot(c, slot, B);
    if (rc) return rc;
    const Slot& s = c->slot[slot];
    if (B > std::max(0, s.records)) return fail(c, IRLOSC_ERR_STATE, "slot %d holds state for %d instances", slot, std::max(0, s.records));
    if (B == 0) return IRLOSC_OK;
    HIPCHK(c, hipSetDevice(c->cfg.hip_device));
    const size_t b = (size_t)B, n = (size_t)c->cfg.n, k = (size_t)c->k, nd = (size_t)c->cfg.ndev, e = c->esz;
    if (M) HIPCHK(c, hipMemcpyAsync(M, s.M, b * n * n * e, hipMemcpyDeviceToHost, c->stream));
    if (J) HIPCHK(c, hipMemcpyAsync(J, s.J, b * k * n * e, hipMemcpyDeviceToHost, c->stream));
    if (dq) HIPCHK(c, hipMemcpyAsync(dq, s.dq, b * n * e, hipMemcpyDeviceToHost, c->stream));
    if (bias) HIPCHK(c, hipMemcpyAsync(bias, s.bias, b * n * e, hipMemcpyDeviceToHost, c->stream));
    if (ee_pose) HIPCHK(c, hipMemcpyAsync(ee_pose, s.ee, b * nd * 7 * e, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return IRLOSC_OK;
}

// A step from joint coordinates over B robots needs B robots of (qpos, qvel) AND of targets in the slot.
static int check_slot_q(irlosc_ctx* c, int slot, int B) {
    if (!c->model.in_force) return fail(c, IRLOSC_ERR_STATE, "irlosc_set_model has not been called");
    const Slot& s = c->slot[slot];
    if (!s.coords || !s.targets)
        return fail(c, IRLOSC_ERR_STATE, "slot %d: irlosc_upload_q and irlosc_set_targets must precede a step from joint coordinates", slot);
    if (B > std::max(0, s.coords) || B > std::max(0, s.targets))
        return fail(c, IRLOSC_ERR_STATE, "slot %d holds joint coordinates of %d and targets for %d instances, step asked for %d", slot,
                    std::max(0, s.coords), std::max(0, s.targets), B);
    return IRLOSC_OK;
}

// A step from joint coordinates over B robots of a slot with a sensor feed needs B robots of sensordata in it.
static int check_slot_feed(irlosc_ctx* c, int slot, int B) {
    const int feed = c->slot[slot].feed;
    if (feed > 0 && B > feed) return fail(c, IRLOSC_ERR_STATE, "slot %d: the sensor feed holds %d robots, step asked for %d", slot, feed, B);
    return IRLOSC_OK;
}

// The wrench of the sensor feed for the n steps s[0 .. n) of a train (those whose slot has a feed): one launch, blockIdx.y = step.
static int ft_launch(irlosc_ctx* c, const FtStep* s, int n, int B, hipStream_t st) {
    if (n < 1 || B < 1) return IRLOSC_OK;
    FtTrain tr;
    memset(&tr, 0, sizeof tr);
    for (int i = 0; i < n; ++i) tr.s[i] = s[i];
    for (int d = 0; d < c->cfg.ndev; ++d) {
        tr.f0[d] = c->ft_f0[d]; tr.t0[d] = c->ft_t0[d]; tr.qe[d] = c->model.ft_qe[d];
        for (int i = 0; i < 9; ++i) tr.R[d][i] = c->ft_R[d][i];
    }
    tr.B = B; tr.ndev = c->cfg.ndev; tr.n_sensor = c->ft_n_sensor; tr.n_entries = (int32_t)c->model.fe_xentries;
    HIPCHK(c, (hipError_t)(c->cfg.dtype == IRLOSC_F64 ? launch_ft_wrench<double>(tr, n, st) : launch_ft_wrench<float>(tr, n, st)));
    return IRLOSC_OK;
}

// The wrench buffer of step i of bank k's trains for a slot with a sensor feed (nullptr: out of device memory)
static void* feed_wrench(irlosc_ctx* c, int k, int i) {
    DevBuf<void>& w = c->bank[k].ftw[i];
    if (!got(w.ensure((size_t)c->cfg.max_batch * c->cfg.ndev * 6 * c->esz))) {
        fail(c, IRLOSC_ERR_HIP, "out of device memory for the wrench of the sensor feed");
        return nullptr;
    }
    return w;
}

// Bank 0 ready for a fused train of n steps, under the fused path's out-of-memory policy: without exchange buffers the path is switched
// off for this context and the caller continues through dense records (-> false); without lane records the OSC step stays the row16
// FROMQ kernel.  (A caller of irlosc_step_from_q needs one step's buffers, the benchmark form R16_TRAIN: 1.4 GB of exchange buffers at
// 65 536 robots -- a context that only ever runs irlosc_frontend + irlosc_step pays nothing.)
static bool fused_ready(irlosc_ctx* c, int n) {
    if (from_q_form(c, false) == FROMQ_DENSE) return false;
    const unsigned miss = ensure_bank(c, 0, n, fused_need(c));
    if (miss == NEED_X) c->model.give_up_fused(c);
    if (miss == NEED_LANE) c->model.give_up_lane(c);
    return from_q_form(c, false) != FROMQ_DENSE;
}

// irlosc_rollout_from_q: the plant kernel behind the step (one step on bank 0), handed to the next train like the timing events
// (irlosc_ctx::plant_next); trace: the device sample of this tick's EE poses, or nullptr.  What else the tick runs, and as which
// tick, is the slot's to say (Slot::prog).  log: the episode log's sample of this tick (irlosc_rollout_from_q_logged), or nullptr.
// A logged tick: the ring's sample it fills, the event its first log launch waits for on the tick's stream (the half it starts was still
// draining: the copy that empties it; else null), and what stays the same over the call -- channels, robots (device, or nullptr: all), layout
struct LogCall { double* sample; hipEvent_t wait; uint32_t channels; const int32_t* robots; int32_t R; int64_t off[LOG_CHANNELS]; };      // (off[9]: OBJECT_POSE, of a slot with objects; off[10], off[11]: of a slot with a policy; off[12]: of one with a reward)
struct PlantCall { double* trace; const LogCall* log; };

// The exchange entry of each device's EE pose (its x; y z qw qx qy qz follow): what the rollout's kernels find an EE body by
static void fill_ee0(const irlosc_ctx* c, int32_t* ee0) { for (int d = 0; d < c->cfg.ndev; ++d) ee0[d] = c->model.tables.eetab[d][0]; }

// The arguments of the slot's action kernel over B robots (init: the launch of irlosc_set_action_list; else a tick on exchange block xside)
static ActionArgs action_args(const irlosc_ctx* c, const Slot& s, int B, const irlosc_action_list& d, const double* xside, int tick) {
    const Program& p = s.prog;
    ActionArgs a;
    memset(&a, 0, sizeof a);
    const size_t Bm = (size_t)c->cfg.max_batch;
    a.xside = xside; a.tgt = s.tgt; a.gains = p.al_gains; a.st = p.list_state(Bm); a.table = p.al_table;
    if (xside && p.refs && s.objects.robots) {      // (refs live only next to the objects they name: irlosc_set_objects ends them)
        a.obj_pose = s.objects.state(Bm).pose;
        for (int i = 0; i < d.n_actions; ++i) { a.xyz_obj[i] = (int8_t)p.rf.xyz_obj[i]; a.quat_obj[i] = (int8_t)p.rf.quat_obj[i]; }
    }
    for (int i = 0; i < d.n_actions; ++i) {
        a.kp[i] = d.kp[i]; a.max_error[i] = d.max_error[i]; a.min_speed[i] = d.min_speed[i]; a.max_speed[i] = d.max_speed[i];
        a.force[i] = d.gripper_force[i]; a.grip_ticks[i] = d.grip_ticks[i];
        a.kind[i] = (uint8_t)d.kind[i]; a.xyz_from_start[i] = (uint8_t)d.xyz_from_start[i];
    }
    for (int i = 0; i < 4; ++i) a.passive_quat[i] = d.passive_quat[i];
    for (int i = 0; i < 7 && xside; ++i) {
        a.ee_act[i] = c->model.tables.eetab[d.active_dev][i];
        a.ee_pas[i] = d.passive_dev >= 0 ? c->model.tables.eetab[d.passive_dev][i] : 0;
    }
    a.B = B; a.ndev = c->cfg.ndev; a.stride = (int32_t)Bm; a.A = d.n_actions; a.per_robot = d.nb > 1;
    a.n_entries = (int32_t)c->model.fe_xentries; a.tick = tick; a.init = xside ? 0 : 1;
    a.active = d.active_dev; a.passive = d.passive_dev; a.hold = d.passive_hold_orientation;
    return a;
}

// ... of a tick of a slot whose list has a motion: the list's, and the motion in force with its state
static ActionMotionArgs action_motion_args(const irlosc_ctx* c, const Slot& s, int B, const double* xside, int tick) {
    const Program& p = s.prog;
    ActionMotionArgs a;
    memset(&a, 0, sizeof a);
    static_cast<ActionArgs&>(a) = action_args(c, s, B, p.al, xside, tick);
    a.mo = p.motion_state((size_t)c->cfg.max_batch);
    for (int i = 0; i < p.al.n_actions; ++i) { a.steps[i] = p.am.steps[i]; a.noise_mean[i] = p.am.noise_mean[i]; a.noise_std[i] = p.am.noise_std[i]; }
    a.seed = p.am.seed;
    return a;
}

// The arguments of the slot's object kernel over B robots for description d (init: the launch of irlosc_set_objects, d not in force yet;
// else a tick on exchange block xside)
static ObjectArgs object_args(const irlosc_ctx* c, const Slot& s, int B, const irlosc_objects& d, const double* xside) {
    const Objects& o = s.objects;
    ObjectArgs a;
    memset(&a, 0, sizeof a);
    const size_t Bm = (size_t)c->cfg.max_batch;
    a.xside = xside; a.qt = s.qt; a.pose0 = o.table; a.st = o.state(Bm);
    for (int g = 0; g < d.n_grippers; ++g) {
        a.sign[g] = (double)d.sign[g]; a.q_close[g] = d.q_close[g]; a.q_open[g] = d.q_open[g]; a.joint[g] = d.joint[g];
        for (int i = 0; i < 3; ++i) a.grip_xyz[g][i] = d.grip_xyz[g][i];
        for (int i = 0; i < 7 && xside; ++i) a.ee[g][i] = c->model.tables.eetab[d.dev[g]][i];
    }
    for (int i = 0; i < d.n_objects; ++i) a.radius[i] = d.radius[i];
    for (int m = 0; m < d.n_mates; ++m) {
        a.plug[m] = d.plug[m]; a.socket[m] = d.socket[m]; a.tol_xyz[m] = d.tol_xyz[m]; a.min_abs_dot[m] = d.min_abs_dot[m];
        for (int i = 0; i < 3; ++i) a.seat_xyz[m][i] = d.seat_xyz[m][i];
        for (int i = 0; i < 4; ++i) a.seat_quat[m][i] = d.seat_quat[m][i];
    }
    a.B = B; a.n = c->cfg.n; a.stride = (int32_t)Bm; a.nobj = d.n_objects; a.ng = d.n_grippers; a.nm = d.n_mates;
    a.n_entries = (int32_t)c->model.fe_xentries; a.tick = o.tick; a.init = xside ? 0 : 1;
    return a;
}

// The arguments of the slot's stream kernel over B robots: a tick on reading `index` of stream d, or (index < 0) the init launch of
// irlosc_set_teleop_stream, which takes the origins (per robot: at ts_origin; shared: `shared`) where a tick takes the readings
static TeleopArgs teleop_args(const irlosc_ctx* c, const Slot& s, int B, const irlosc_teleop_stream& d, const double* shared, int index) {
    const Program& p = s.prog;
    TeleopArgs a;
    memset(&a, 0, sizeof a);
    const size_t Bm = (size_t)c->cfg.max_batch;
    a.init = index < 0;
    a.per_robot = (a.init ? d.nb_origin : d.nb) > 1;
    a.tgt = s.tgt; a.st = p.plate_state(Bm); a.readings = a.init ? p.ts_origin : p.ts_table;
    for (int i = 0; i < 6 && !a.per_robot; ++i) a.r[i] = shared[(a.init ? 0 : (size_t)index * 6) + i];
    a.inc = d.increment;
    for (int k = 0; k < c->cfg.ndev; ++k) {
        a.kind[k] = d.kind[k]; a.heading[k] = d.heading_offset[k];
        for (int i = 0; i < 3; ++i) a.off_xyz[k][i] = d.off_xyz[k][i];
        for (int i = 0; i < 4; ++i) a.off_quat[k][i] = d.off_quat[k][i];
    }
    a.B = B; a.ndev = c->cfg.ndev; a.stride = (int32_t)Bm; a.T = d.ticks; a.index = a.init ? 0 : index;
    return a;
}

// The arguments of the slot's policy kernel over B robots: a tick on exchange block xside, wrench: the feed's wrench of the tick (or nullptr)
static PolicyArgs policy_args(const irlosc_ctx* c, const Slot& s, int B, const double* xside, const void* wrench) {
    const Program& p = s.prog;
    PolicyArgs a;
    memset(&a, 0, sizeof a);
    const size_t Bm = (size_t)c->cfg.max_batch;
    a.t = teleop_args(c, s, B, p.ts, p.po_origin0, 0);      // (the rig, the targets, the pose; no reading: the kernel computes it)
    a.net = p.po_net; a.w = p.po_w; a.qt = s.qt; a.xside = xside; a.wrench = wrench; a.obj_pose = s.objects.state(Bm).pose;
    a.st = p.policy_state(); a.obs = p.po.keep_obs ? p.po_obs.get() : nullptr; a.flags_any = c->dflags_any;
    a.grip_close = p.po.grip_close; a.grip_open = p.po.grip_open; a.clip = p.po.clip; a.obs_mask = p.po.obs;
    if (p.noise) { a.seed = p.pn.seed; a.logp_const = p.pn_const; for (int i = 0; i < 8; ++i) a.std[i] = p.pn.std[i]; }
    a.n = c->cfg.n; a.n_entries = (int32_t)c->model.fe_xentries; a.nobj = std::max(0, p.po_nobj);
    fill_ee0(c, a.ee0);
    return a;
}

// The arguments of the slot's waypoint cycler over B robots (init: the launch of irlosc_set_waypoints; else a tick on exchange block xside)
static WaypointArgs waypoint_args(const irlosc_ctx* c, const Slot& s, int B, const irlosc_waypoints& w, const double* xside, int tick) {
    WaypointArgs a;
    memset(&a, 0, sizeof a);
    const Program& p = s.prog;
    const size_t plane = (size_t)c->cfg.ndev * c->cfg.max_batch;
    a.xside = xside; a.tgt = s.tgt; a.table = p.wp_table; a.st = p.path_state(plane);
    for (int d = 0; d < c->cfg.ndev; ++d) {
        a.thr2[d] = w.threshold[d] * w.threshold[d];
        a.count[d] = w.count[d];
        a.loop[d] = w.loop[d];
        a.wmax = std::max(a.wmax, w.count[d]);      // the widest list: the table's stride
    }
    if (xside) fill_ee0(c, a.ee0);      // (the init launch reads no block)
    a.B = B; a.ndev = c->cfg.ndev; a.stride = c->cfg.max_batch; a.per_robot = w.nb > 1;
    a.n_entries = (int32_t)c->model.fe_xentries; a.tick = tick; a.init = xside ? 0 : 1;
    return a;
}

// The arguments of the slot's push kernel over B robots: the pushes of `active`, applied to exchange block xside or (xside == nullptr)
// taken off the feed's wrench
static PushArgs push_args(const irlosc_ctx* c, const Slot& s, int B, uint32_t active, double* xside, void* wrench) {
    const Pushes& p = s.push;
    PushArgs a;
    memset(&a, 0, sizeof a);
    a.xside = xside; a.wrench = wrench; a.table = p.table;
    a.B = B; a.ndev = c->cfg.ndev; a.P = p.d.n_pushes; a.per_robot = p.d.nb > 1;
    a.apply = xside ? 1 : 0; a.active = active;
    for (int i = 0; i < p.d.n_pushes; ++i) a.dev[i] = p.d.dev[i];
    fill_ee0(c, a.ee0);
    return a;
}

// The arguments of the slot's wall kernel over B robots: the devices of `devs`, applied to exchange block xside or (xside == nullptr)
// their stored force taken off the feed's wrench
static WallArgs wall_args(const irlosc_ctx* c, const Slot& s, int B, uint32_t devs, double* xside, void* wrench) {
    const Walls& w = s.walls;
    const size_t plane = (size_t)c->cfg.ndev * c->cfg.max_batch;
    WallArgs a;
    memset(&a, 0, sizeof a);
    a.xside = xside; a.qt = s.qt; a.wrench = wrench; a.table = w.table; a.st = w.state(plane);
    a.B = B; a.ndev = c->cfg.ndev; a.W = w.d.n_walls; a.per_robot = w.d.nb > 1; a.stride = c->cfg.max_batch;
    a.apply = xside ? 1 : 0; a.tick = w.tick; a.devs = devs;
    for (int i = 0; i < w.d.n_walls; ++i) a.dev[i] = w.d.dev[i];
    fill_ee0(c, a.ee0);
    return a;
}

// The arguments of the slot's load kernel over B robots: the grippers of `grippers`, their weight applied to exchange block xside or
// (xside == nullptr) their stored load taken off the feed's wrench
static ObjectLoadArgs load_args(const irlosc_ctx* c, const Slot& s, int B, uint32_t grippers, double* xside, void* wrench) {
    const Loads& l = s.loads;
    const Objects& o = s.objects;
    const size_t Bm = (size_t)c->cfg.max_batch;
    ObjectLoadArgs a;
    memset(&a, 0, sizeof a);
    a.xside = xside; a.wrench = wrench; a.table = l.table;
    a.obj_pose = o.state(Bm).pose; a.obj_holder = o.state(Bm).holder; a.st = l.state(Bm);
    for (int i = 0; i < 3; ++i) a.gravity[i] = l.d.gravity[i];
    a.B = B; a.ndev = c->cfg.ndev; a.nobj = o.d.n_objects; a.ng = o.d.n_grippers; a.per_robot = l.d.per_robot; a.stride = (int32_t)Bm;
    a.apply = xside ? 1 : 0; a.grippers = grippers;
    for (int g = 0; g < o.d.n_grippers; ++g) a.dev[g] = o.d.dev[g];
    fill_ee0(c, a.ee0);
    return a;
}

// The arguments of the slot's joint-row kernel over B robots on exchange block xside: per hinge the rows that name it, in ascending row
// (the accumulation order of osc_joint.hpp), and the ACTION drives that the list in force arms on this tick
static JointArgs joint_args(const irlosc_ctx* c, const Slot& s, int B, double* xside) {
    const Joints& j = s.joints;
    const irlosc_joint_rows& d = j.d;
    const size_t Bm = (size_t)c->cfg.max_batch, n = (size_t)c->cfg.n;
    JointArgs a;
    memset(&a, 0, sizeof a);
    a.xside = xside; a.qt = s.qt; a.table = j.table; a.st = j.state(Bm);
    a.B = B; a.R = d.n_rows; a.per_robot = d.per_robot; a.stride = (int32_t)Bm;
    const bool list = s.prog.kind == Program::LIST, grips = s.prog.kind == Program::POLICY && s.prog.po.n_out == 7;
    a.gripper_force = list ? s.prog.list_state(Bm).gripper_force : grips ? s.prog.policy_state().grip : nullptr;      // (the list's own state, or the policy's grip: what its ACTION drives read)
    int items = 0;
    for (int h = 0; h < (int)n; ++h) {
        a.first[h] = (uint8_t)items;
        for (int r = 0; r < d.n_rows; ++r) {
            if (d.joint_a[r] == h) a.item[items++] = (uint8_t)r;
            else if (d.kind[r] == IRLOSC_JOINT_COUPLE && d.joint_b[r] == h) a.item[items++] = (uint8_t)(r | 0x80);
        }
    }
    for (int h = (int)n; h <= IRLOSC_MAX_N; ++h) a.first[h] = (uint8_t)items;
    for (int r = 0; r < d.n_rows; ++r) {
        a.kind[r] = (uint8_t)d.kind[r]; a.ja[r] = (uint8_t)d.joint_a[r]; a.jb[r] = (uint8_t)d.joint_b[r]; a.source[r] = (uint8_t)d.source[r];
        if ((list || grips) && d.kind[r] == IRLOSC_JOINT_DRIVE && d.source[r] == IRLOSC_JOINT_SRC_ACTION && d.dev[r] == (list ? s.prog.al.active_dev : s.prog.po.grip_dev))
            a.armed |= (uint64_t)1 << r;
    }
    return a;
}

// The arguments of the plant kernel behind the tick's step on bank bk over B robots (trace: the device sample of its EE poses, or nullptr)
static PlantArgs plant_args(const irlosc_ctx* c, const Slot& s, int B, const irlosc_ctx::Bank& bk, double* trace) {
    PlantArgs a;
    memset(&a, 0, sizeof a);
    a.xside = bk.xside[0]; a.u = bk.u[0]; a.flags = bk.flags[0]; a.qt = s.qt; a.qpos = s.qpos; a.qvel = s.qvel;
    a.trace = trace; a.flags_any = c->dflags_any; a.dt = c->plant.dt; a.damping = c->plant.damping; a.ctrl_mask = c->plant.ctrl_mask;
    a.B = B; a.ndev = c->cfg.ndev; fill_ee0(c, a.ee0);
    return a;
}

// The arguments of a log launch of the tick's step on bank bk: the channels of `mask` out of the log's (the front or the back ones; none: no
// launch), wrench: the feed's wrench of the tick (or nullptr: the slot has no feed, and the log no WRENCH channel)
static LogArgs log_args(const irlosc_ctx* c, const Slot& s, const irlosc_ctx::Bank& bk, const LogCall& lg, uint32_t mask, const void* wrench) {
    LogArgs a;
    memset(&a, 0, sizeof a);
    const size_t Bm = (size_t)c->cfg.max_batch;
    a.sample = lg.sample; a.robots = lg.robots; a.mask = lg.channels & mask;
    for (int i = 0; i < LOG_CHANNELS; ++i) a.off[i] = lg.off[i];
    a.qpos = s.qpos; a.qvel = s.qvel; a.xside = bk.xside[0]; a.tgt = s.tgt; a.wrench = wrench; a.u = bk.u[0]; a.flags = bk.flags[0];
    a.wall_force = s.walls.state((size_t)c->cfg.ndev * Bm).force; a.joint_tau = s.joints.state(Bm).tau;
    a.obj_pose = s.objects.state(Bm).pose; a.obj_holder = s.objects.state(Bm).holder; a.nobj = s.objects.count();
    if (s.prog.kind == Program::POLICY) { const PolicyState po = s.prog.policy_state(); a.po_out = po.out; a.po_act = po.act; a.po_logp = po.logp; a.n_out = s.prog.po.n_out; }
    if (s.reward.robots) { const RewardState rw = s.reward.state(Bm); a.rw_r = rw.r; a.rw_ret = rw.ret; a.rw_steps = rw.steps; a.rw_goal_step = rw.goal_step; }
    a.R = lg.R; a.n = c->cfg.n; a.ndev = c->cfg.ndev; a.n_entries = (int32_t)c->model.fe_xentries; a.stride = (int32_t)Bm;
    fill_ee0(c, a.ee0);
    return a;
}

// The arguments of the slot's reward kernel over B robots for description d with its points laid out per_robot or not: a tick of the
// step on bank bk (wrench: the feed's wrench of the tick, or nullptr), or (bk == nullptr) the init launch of irlosc_set_reward
static RewardArgs reward_args(const irlosc_ctx* c, const Slot& s, int B, const irlosc_reward& d, int per_robot, const irlosc_ctx::Bank* bk, const void* wrench) {
    const Reward& w = s.reward;
    const Program& p = s.prog;
    const size_t Bm = (size_t)c->cfg.max_batch;
    RewardArgs a;
    memset(&a, 0, sizeof a);
    a.st = w.state(Bm);
    a.B = B; a.n = c->cfg.n; a.ndev = c->cfg.ndev; a.stride = (int32_t)Bm; a.init = bk ? 0 : 1;
    if (!bk) return a;
    a.xside = bk->xside[0]; a.tgt = s.tgt; a.u = bk->u[0]; a.wrench = wrench;
    a.obj_pose = s.objects.state(Bm).pose; a.mated_tick = s.objects.state(Bm).mated_tick;
    if (p.kind == Program::POLICY) { const PolicyState po = p.policy_state(); a.act = po.act ? po.act : po.out; a.n_out = p.po.n_out; }
    a.points = w.table; a.per_robot = per_robot;
    for (int i = 0; i < d.n_terms; ++i) {
        a.weight[i] = d.weight[i]; a.kind[i] = (int8_t)d.kind[i];
        a.a_kind[i] = (int8_t)d.a_kind[i]; a.a_index[i] = (int8_t)d.a_index[i]; a.b_kind[i] = (int8_t)d.b_kind[i]; a.b_index[i] = (int8_t)d.b_index[i];
        const bool pts = d.kind[i] == IRLOSC_REWARD_DIST_SQ || d.kind[i] == IRLOSC_REWARD_DIST || d.kind[i] == IRLOSC_REWARD_ORI;
        if (pts && (d.a_kind[i] == IRLOSC_REWARD_TARGET || d.b_kind[i] == IRLOSC_REWARD_TARGET)) a.need |= REWARD_NEED_TGT;
        if (d.kind[i] == IRLOSC_REWARD_U_SQ) a.need |= REWARD_NEED_U;
        if (d.kind[i] == IRLOSC_REWARD_FORCE) a.need |= REWARD_NEED_WRENCH;
    }
    a.gamma = d.gamma; a.goal_value = d.goal_value;
    a.n_terms = d.n_terms; a.P = d.n_points; a.goal_term = d.goal_term; a.goal_cmp = d.goal_cmp; a.goal_hold = d.goal_hold;
    a.n_entries = (int32_t)c->model.fe_xentries;
    fill_ee0(c, a.ee0);
    return a;
}

// What reward d names, the slot has for B robots: asked by irlosc_set_reward of the description it is given, and by every rollout call of
// the reward in force (parts come and go behind a reward's back).  IRLOSC_ERR_STATE with the reason.
static int check_reward_refs(irlosc_ctx* c, int slot, int B, const irlosc_reward& d) {
    const Slot& s = c->slot[slot];
    if (!c->model.in_force) return fail(c, IRLOSC_ERR_STATE, "irlosc_set_model has not been called");
    if (c->cfg.n != plant_joints()) return fail(c, IRLOSC_ERR_STATE, "no reward on this context: the rollout's kernels hold %d joints, n=%d", plant_joints(), c->cfg.n);
    if (B > std::max(0, s.targets))
        return fail(c, IRLOSC_ERR_STATE, "slot %d holds targets for %d instances, its reward covers %d: irlosc_set_targets first", slot, std::max(0, s.targets), B);
    for (int i = 0; i < d.n_terms; ++i) {
        const int kind = d.kind[i];
        const bool pts = kind == IRLOSC_REWARD_DIST_SQ || kind == IRLOSC_REWARD_DIST || kind == IRLOSC_REWARD_ORI;
        for (int h = 0; pts && h < 2; ++h) {
            const int pk = h ? d.b_kind[i] : d.a_kind[i], pi = h ? d.b_index[i] : d.a_index[i];
            if (pk == IRLOSC_REWARD_OBJECT && (pi >= s.objects.count() || s.objects.robots < B))
                return fail(c, IRLOSC_ERR_STATE, "slot %d: term %d of its reward reads action object %d of %d robots, the slot has %d objects of %d (irlosc_set_objects)", slot,
                            i, pi, B, s.objects.count(), s.objects.robots);
        }
        if (kind == IRLOSC_REWARD_MATED && (s.objects.robots < B || d.a_index[i] >= (s.objects.robots ? s.objects.d.n_mates : 0)))
            return fail(c, IRLOSC_ERR_STATE, "slot %d: term %d of its reward reads mate %d of %d robots, the slot has %d mates of %d (irlosc_set_objects)", slot, i,
                        d.a_index[i], B, s.objects.robots ? s.objects.d.n_mates : 0, s.objects.robots);
        if (kind == IRLOSC_REWARD_ACT_SQ && (s.prog.kind != Program::POLICY || s.prog.robots < B))
            return fail(c, IRLOSC_ERR_STATE, "slot %d: term %d of its reward reads a policy's action of %d robots, the slot has %s (irlosc_set_policy)", slot, i, B,
                        s.prog.kind == Program::POLICY ? "one for fewer" : "no policy");
        if (kind == IRLOSC_REWARD_FORCE && (s.feed < B || c->ft_f0[d.a_index[i]] < 0))
            return fail(c, IRLOSC_ERR_STATE, "slot %d: term %d of its reward reads the sensed force of device %d of %d robots, %s (irlosc_set_sensordata)", slot, i,
                        d.a_index[i], B, s.feed < B ? "the slot's sensor feed covers fewer" : "the feed has no force sensor for that device");
    }
    return IRLOSC_OK;
}

// The arguments of the slot's episode kernel over B robots: a tick (the program, walls and rows in force on it travel as uniform arguments)
// or, with init, the launch of irlosc_set_episodes for description d, which is not in force yet
static EpisodeArgs episode_args(const irlosc_ctx* c, const Slot& s, int B, const irlosc_episodes& d, bool init) {
    const Episodes& e = s.episodes;
    const Program& p = s.prog;
    const size_t Bm = (size_t)c->cfg.max_batch, plane = (size_t)c->cfg.ndev * Bm;
    EpisodeArgs a;
    memset(&a, 0, sizeof a);
    a.count = e.count(Bm); a.age = e.age(Bm); a.start_tick = e.start_tick(Bm); a.ring = e.ring(Bm); a.running = e.running;
    a.qt = s.qt; a.qpos = s.qpos; a.qvel = s.qvel; a.starts = e.starts; a.tgt = s.tgt; a.snap = e.snap;
    a.kind = p.kind == Program::LIST ? EP_LIST : p.kind == Program::PATHS ? EP_PATHS : p.kind == Program::POLICY ? EP_POLICY : EP_NONE;
    if (a.kind == EP_POLICY) {
        a.pl = p.plate_state(Bm); a.pl_origin = p.po.nb_origin > 1 ? p.ts_origin.get() : nullptr; a.po = p.policy_state(); a.pl_n_out = p.po.n_out;
        for (int i = 0; i < 6; ++i) a.pl_origin0[i] = p.po_origin0[i];
    }
    if (a.kind == EP_LIST) {
        a.ls = p.list_state(Bm); a.al_table = p.al_table; a.variants = e.variants; a.al_gains = p.al_gains; a.gains = c->dgains;
        a.A = p.al.n_actions; a.active = p.al.active_dev; a.gains_per_robot = c->gains_nb > 1;
        a.V = d.n_variants; a.vstride = (int64_t)e.vstride; a.list_per_robot = e.list_per_robot;
    }
    if (a.kind == EP_PATHS) {
        a.wp = p.path_state(plane); a.wp_table = p.wp_table;
        for (int k = 0; k < c->cfg.ndev; ++k) {
            a.wp_count[k] = p.wp.count[k]; a.wp_loop[k] = p.wp.loop[k];
            a.wmax = std::max(a.wmax, p.wp.count[k]);
        }
        a.wp_per_robot = p.wp.nb > 1;
    }
    if (!init && s.walls.robots) { a.walls = 1; a.wl = s.walls.state(plane); }
    if (!init && s.joints.robots) { a.joints = 1; a.R = s.joints.d.n_rows; a.jt = s.joints.state(Bm); }
    if (!init && s.objects.robots) {
        const Objects& o = s.objects;
        a.objects = 1; a.nobj = o.d.n_objects; a.ng = o.d.n_grippers; a.nm = o.d.n_mates; a.OV = o.d.n_variants;
        a.ob = o.state(Bm); a.ob_pose0 = o.table; a.ob_vstride = (int64_t)o.vstride;
    }
    if (!init && s.loads.robots) { a.loads = 1; a.ld = s.loads.state(Bm); }
    if (!init && s.reward.robots) { a.reward = 1; a.goal = s.reward.goal() ? 1 : 0; a.rw = s.reward.state(Bm); }
    a.B = B; a.ndev = c->cfg.ndev; a.stride = (int32_t)Bm; a.S = d.n_starts; a.starts_per_robot = e.starts_per_robot;
    a.max_ticks = d.max_ticks; a.end_on_finish = d.end_on_finish; a.max_episodes = d.max_episodes; a.records = d.records;
    a.tick = e.tick; a.init = init ? 1 : 0;
    return a;
}

// What the slot has of one part (`robots` of `what`; 0: none) covers B robots.  With `setter` (a download) a slot that has none is refused,
// by the name of the entry point that sets it; without (a rollout) it passes.
static int check_covers(irlosc_ctx* c, int slot, int B, int robots, const char* what, const char* covers, const char* setter) {
    if (setter && !robots) return fail(c, IRLOSC_ERR_STATE, "slot %d has no %s (%s)", slot, what, setter);
    if (robots && B > robots)
        return fail(c, IRLOSC_ERR_STATE, "slot %d: its %s %s %d robots, %sasked for %d", slot, what, covers, robots, setter ? "" : "rollout ", B);
    return IRLOSC_OK;
}

// The slot's program covers B robots and, with `need` (a download), is of that kind; without (a rollout) a slot that has none passes
static int check_program(irlosc_ctx* c, int slot, int B, Program::Kind need = Program::NONE) {
    static const char* const what[] = {"", "waypoint paths", "action list", "teleoperation stream", "policy"};      // by Program::Kind
    static const char* const covers[] = {"", "cover", "covers", "covers", "covers"};
    static const char* const setter[] = {"", "irlosc_set_waypoints", "irlosc_set_action_list", "irlosc_set_teleop_stream", "irlosc_set_policy"};
    const Program& p = c->slot[slot].prog;
    const Program::Kind k = need ? need : p.kind;
    return check_covers(c, slot, B, !need || p.kind == need ? p.robots : 0, what[k], covers[k], need ? setter[k] : nullptr);
}

// A policy that observes the action objects finds those it was sized for, for B robots (objects come and go behind a policy's back)
static int check_policy_objects(irlosc_ctx* c, int slot, int B) {
    const Slot& s = c->slot[slot];
    if (s.prog.kind != Program::POLICY || s.prog.po_nobj < 0) return IRLOSC_OK;
    if (s.objects.count() != s.prog.po_nobj || s.objects.robots < B)
        return fail(c, IRLOSC_ERR_STATE, "slot %d: its policy observes %d action objects of %d robots, the slot has %d of %d (irlosc_set_policy again)", slot,
                    s.prog.po_nobj, B, s.objects.count(), s.objects.robots);
    return IRLOSC_OK;
}

// A program's table [nb][E] in the layout its kernel walks: per robot [walk wave][E][64] (idle lanes zero), shared (nb == 1) as given
static std::vector<double> walk_table(const double* t, int nb, size_t E) {
    std::vector<double> tab(nb == 1 ? E : ((size_t)nb + 63) / 64 * E * 64, 0.0);
    for (int b = 0; b < nb; ++b)
        for (size_t e = 0; e < E; ++e) tab[nb == 1 ? e : ((size_t)(b / 64) * E + e) * 64 + b % 64] = t[(size_t)b * E + e];
    return tab;
}

// The tail of every setter of a program or of what acts on the plant: host arrays to the device and fills with a byte value (src == nullptr)
// as listed (one of no bytes -- a table that stays on the host -- is skipped), then the init launch of a program's kernel if given, on the context's stream -> the first error.  Synchronises also when one of
// them failed: the host arrays are the copies' sources.  Only then does the caller bring the part in force.
struct Upload { void* dst; const void* src; size_t bytes; int byte; };
template <typename Args = int>
static int setter_upload(irlosc_ctx* c, std::initializer_list<Upload> ups, int (*init)(const Args&, hipStream_t) = nullptr, const Args* a = nullptr) {
    hipError_t ec = hipSuccess;
    for (const Upload& k : ups)
        if (ec == hipSuccess && k.bytes) ec = k.src ? hipMemcpyAsync(k.dst, k.src, k.bytes, hipMemcpyHostToDevice, c->stream) : hipMemsetAsync(k.dst, k.byte, k.bytes, c->stream);
    if (ec == hipSuccess && init) ec = (hipError_t)init(*a, c->stream);
    const hipError_t es = hipStreamSynchronize(c->stream);
    HIPCHK(c, ec);
    HIPCHK(c, es);
    return IRLOSC_OK;
}

// A download of per-robot state: `nd` doubles at sd and `ni` ints at si (either may be 0) to the host, one synchronise, then every Gather: row
// p of the `count` rows [max_batch] from `src` on (the owner's accessor) goes to dst[b * ld + off + p * step], b < B (dst == NULL: skipped)
template <typename T> struct Gather { T* dst; const T* src; size_t count, ld, off, step; };
static int download_state(irlosc_ctx* c, int B, const double* sd, size_t nd, std::initializer_list<Gather<double>> gd, const int32_t* si,
                          size_t ni, std::initializer_list<Gather<int32_t>> gi) {
    std::vector<double> hd(nd);  std::vector<int32_t> hi(ni);
    if (nd) HIPCHK(c, hipMemcpyAsync(hd.data(), sd, hd.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (ni) HIPCHK(c, hipMemcpyAsync(hi.data(), si, hi.size() * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const size_t Bm = (size_t)c->cfg.max_batch;
    auto gather = [&](const auto& h, const auto* dev, const auto& to) {
        for (const auto& g : to)
            for (size_t b = 0; g.dst && b < (size_t)B; ++b)
                for (size_t p = 0; p < g.count; ++p) g.dst[b * g.ld + g.off + p * g.step] = h[(size_t)(g.src - dev) + p * Bm + b];
    };
    gather(hd, sd, gd); gather(hi, si, gi);
    return IRLOSC_OK;
}

// What a tick of a rollout runs next to its fused step, decided once per tick from the slot (the default: no tick, nothing): the program that writes its
// targets; the pushes and the walls' devices that act on its plant, and those its sensors read of the tick before (a feed, and the device a sensor); the
// grippers whose carried object weighs on the plant, and those whose device's sensor reads the weight of the tick before; rows
// it has; a stream's reading of the tick (-1: none -- no stream, or one that has ended: no launch, its tick counts on); episodes it has;
// a reward it has
struct TickPlan { Program::Kind prog = Program::NONE; uint32_t push_apply = 0, push_sense = 0, wall_apply = 0, wall_sense = 0; bool joints = false; int reading = -1; bool episodes = false; bool objects = false; uint32_t load_apply = 0, load_sense = 0; bool reward = false; };
static TickPlan tick_plan(const irlosc_ctx* c, const Slot& s0) {
    TickPlan tp{s0.prog.kind, s0.push.applied(), s0.feed > 0 ? s0.push.sensed() : 0u, s0.walls.devices(), 0u, s0.joints.robots != 0, s0.prog.reading(), s0.episodes.robots != 0, s0.objects.robots != 0};
    for (int p = 0; tp.push_sense && p < IRLOSC_MAX_PUSHES; ++p)
        if (((tp.push_sense >> p) & 1u) && c->ft_f0[s0.push.d.dev[p]] < 0) tp.push_sense &= ~(1u << p);
    if (s0.feed > 0 && s0.walls.tick > 0) tp.wall_sense = tp.wall_apply;
    for (int d = 0; tp.wall_sense && d < c->cfg.ndev; ++d)
        if (c->ft_f0[d] < 0) tp.wall_sense &= ~(1u << d);
    for (int g = 0; s0.loads.robots && g < s0.objects.d.n_grippers; ++g) {      // the grippers: bit g
        tp.load_apply |= 1u << g;
        if (s0.feed > 0 && s0.loads.tick > 0 && c->ft_f0[s0.objects.d.dev[g]] >= 0) tp.load_sense |= 1u << g;
    }
    tp.reward = s0.reward.robots != 0;
    return tp;
}

// THE ORDER OF A TICK'S LAUNCHES on the stream of bank 0 ([..]: where the plan has it; the unnamed lines are fused_train's own):
//     the walk, the feed's wrench (ft_launch)
//     tick_front:   [pushes SENSE: their reaction goes into the wrench ahead of every kernel that reads it] [walls SENSE: their force of the
//                   tick before, behind it] [loads SENSE: the carried objects' weight of the tick before, behind that] [action objects: on this tick's EE poses and knuckle coordinates, in front of the action kernel,
//                   whose refs read their poses] [action kernel: its targets and velocity limit are this tick's, so in front of every OSC kernel
//                   | stream kernel: its targets are this tick's too | policy kernel: likewise, and it reads what the launches above left: the wrench behind
//                   every SENSE, the objects' poses of this tick]
//     the OSC kernels (task pass + lane kernel, or row16 FROMQ), the give-up pass (front end over its lists, generic kernel)
//     [reward: behind the give-up pass, which completes u, and directly in front of log FRONT, which can then log it -- so r_t judges the state
//                   the tick observed and the action it took: in front of the cycler, which moves the targets, and of the plant; it reads what the
//                   launches above left (targets, wrench, objects, a policy's action) and writes its own state alone]
//     [log FRONT (a logged tick): coordinates, EE poses, targets, wrench, u and flags as the step used and left them -- behind the give-up
//                   pass, which completes u; in front of the cycler, which moves the targets, and of the plant, which moves the
//                   coordinates and overwrites the block's M entries (the EE entries it leaves alone; the order does not lean on that)]
//     tick_behind:  [waypoint cycler: the targets move where an arm arrived]; [pushes APPLY] [walls APPLY] [loads APPLY: on the holders this tick's object kernel left] [joint rows], each into the bias
//                   entries of the block, which only the plant reads from here on; [log BACK (a logged tick with WALL_FORCE or JOINT_TAU):
//                   the force / tau planes the two launches ahead of it just wrote]; the plant: every robot has its u by then;
//                   [episodes: LAST, because the plant wrote the coordinates that a reset replaces -- and the cycler, the action kernel,
//                   the walls and the rows have judged and recorded the tick whose state a reset wipes]
// The log launches only read, and write nothing but their sample of the ring.
// What rests on this order alone: "pushes, then walls, then loads, then joint rows" on one bias entry of one tick.
template <typename T>
static int tick_front(irlosc_ctx* c, const Slot& s0, int B, const TickPlan& tp, const irlosc_ctx::Bank& bk, void* wrench, hipStream_t st) {
    if (tp.push_sense) HIPCHK(c, (hipError_t)launch_pushes<T>(push_args(c, s0, B, tp.push_sense, nullptr, wrench), st));
    if (tp.wall_sense) HIPCHK(c, (hipError_t)launch_walls<T>(wall_args(c, s0, B, tp.wall_sense, nullptr, wrench), st));
    if (tp.load_sense) HIPCHK(c, (hipError_t)launch_object_loads<T>(load_args(c, s0, B, tp.load_sense, nullptr, wrench), st));
    if (tp.objects) HIPCHK(c, (hipError_t)launch_objects(object_args(c, s0, B, s0.objects.d, bk.xside[0]), st));
    if (tp.prog == Program::LIST && !s0.prog.motion) HIPCHK(c, (hipError_t)launch_actions<T>(action_args(c, s0, B, s0.prog.al, bk.xside[0], s0.prog.tick), st));
    if (tp.prog == Program::LIST && s0.prog.motion) HIPCHK(c, (hipError_t)launch_actions_motion<T>(action_motion_args(c, s0, B, bk.xside[0], s0.prog.tick), st));
    if (tp.reading >= 0) HIPCHK(c, (hipError_t)launch_teleop<T>(teleop_args(c, s0, B, s0.prog.ts, s0.prog.ts_shared.data(), tp.reading), st));
    if (tp.prog == Program::POLICY) HIPCHK(c, (hipError_t)launch_policy<T>(policy_args(c, s0, B, bk.xside[0], wrench), st));
    return IRLOSC_OK;
}
template <typename T>
static int tick_behind(irlosc_ctx* c, const Slot& s0, int B, const TickPlan& tp, const irlosc_ctx::Bank& bk, const PlantCall& pl, hipStream_t st) {
    if (tp.prog == Program::PATHS) HIPCHK(c, (hipError_t)launch_waypoints<T>(waypoint_args(c, s0, B, s0.prog.wp, bk.xside[0], s0.prog.tick), st));
    if (tp.push_apply) HIPCHK(c, (hipError_t)launch_pushes<T>(push_args(c, s0, B, tp.push_apply, bk.xside[0], nullptr), st));
    if (tp.wall_apply) HIPCHK(c, (hipError_t)launch_walls<T>(wall_args(c, s0, B, tp.wall_apply, bk.xside[0], nullptr), st));
    if (tp.load_apply) HIPCHK(c, (hipError_t)launch_object_loads<T>(load_args(c, s0, B, tp.load_apply, bk.xside[0], nullptr), st));
    if (tp.joints) HIPCHK(c, (hipError_t)launch_joints(joint_args(c, s0, B, bk.xside[0]), st));
    if (pl.log && (pl.log->channels & LOG_BACK)) HIPCHK(c, (hipError_t)launch_log<T>(log_args(c, s0, bk, *pl.log, LOG_BACK, nullptr), st));
    HIPCHK(c, (hipError_t)launch_plant<T>(plant_args(c, s0, B, bk, pl.trace), st));
    if (tp.episodes) HIPCHK(c, (hipError_t)launch_episodes<T>(episode_args(c, s0, B, s0.episodes.d, false), st));
    return IRLOSC_OK;
}
// The whole tick is enqueued: the slot's coordinates are the plant's, and what ran is a tick older (a slot without a program ticks none).
static void tick_done(Slot& s0, int B, const TickPlan& tp) { s0.advanced(B); s0.parts_ticked(tp.prog != Program::NONE); }

// irlosc_step_from_q_device: the caller's device arrays and stream in place of the slot's inputs and the bank's outputs (one step)
struct DevCall {
    const double* qpos; const double* qvel;
    const void* tgt; const void* tvel;
    const double* sens;
    void* u; uint32_t* flags;
    hipStream_t st;
};

// Fused path: one train of n steps from joint coordinates (step i: slot slots[i], outputs of set i).  Three launches -- the
// lane-per-robot walk leaves the structural non-zeros of M / J, the bias forces and the EE poses in the compact exchange
// buffer of each step; the task pass (one lane per (robot, device)) adds the k gained task-error rows; the row16 kernel (FROMQ)
// stages a block's lines in LDS and gathers its operands from there -- and, fourth, the give-up pass: the few robots the
// eigen stage hands over get their dense records from the wave-per-robot front end (worklist form) and go through the
// generic kernel like on the record path.  Dense M / J exist in HBM for those robots only.
// With `dv` (one step on bank 0) the caller's arrays replace every per-slot input -- coordinates (the walk reads the slot's dqt, which
// the device entry has laid them out into), targets, sensordata -- and its u / flags the output set; the slot only lends scratch.
// A step whose slot has a sensor feed gets its wrench from the feed (osc_ft_wrench between the walk and the OSC step).
// With `pl` (one step on bank 0 of the slot's own inputs: a tick of irlosc_rollout_from_q) tick_front and tick_behind run around the step (above).
template <typename T>
static int fused_train(irlosc_ctx* c, const int* slots, int n, int B, int k, const DevCall* dv, const PlantCall* pl = nullptr) {
    if (n < 1 || n > R16_TRAIN) return fail(c, IRLOSC_ERR_STATE, "train of %d steps", n);
    if (dv && (n != 1 || k != 0)) return fail(c, IRLOSC_ERR_STATE, "a device-pointer step is one step on bank 0");
    if (pl && (n != 1 || k != 0 || dv)) return fail(c, IRLOSC_ERR_STATE, "a tick of a rollout is one step on bank 0 from the slot's coordinates");
    for (int i = 0; i < n && !dv; ++i) {
        int rc = check_slot_q(c, slots[i], B);
        if (!rc) rc = check_slot_feed(c, slots[i], B);
        if (rc) return rc;
    }
    const irlosc_ctx::Bank& bk = c->bank[k];
    const hipStream_t st = dv ? dv->st : bk.st;
    Slot& s0 = c->slot[slots[0]];      // (the slot of a rollout's tick)
    const TickPlan tp = pl ? tick_plan(c, s0) : TickPlan{};
    FtStep fts[R16_TRAIN];
    int nft = 0;
    FeLaneTrain ft;
    memset(&ft, 0, sizeof ft);
    Row16Train<T> tr;
    memset(&tr, 0, sizeof tr);
    FeGenericArgs<T> ga;
    memset(&ga, 0, sizeof ga);
    HIPCHK(c, hipMemsetAsync(bk.count, 0, R16_TRAIN * sizeof(int32_t), st));
    ft.B = ga.B = B;
    for (int i = 0; i < n; ++i) {
        const Slot& s = c->slot[slots[i]];
        const double* qpos = dv ? dv->qpos : s.qpos;
        const double* qvel = dv ? dv->qvel : s.qvel;
        const double* sens = dv ? dv->sens : s.feed > 0 ? s.sens : nullptr;
        void* wr = !sens ? nullptr : dv ? s.wrench : feed_wrench(c, k, i);      // the feed's wrench (a device call: in the scratch slot)
        if (sens && !wr) return IRLOSC_ERR_HIP;
        if (sens) fts[nft++] = FtStep{sens, wr, bk.xside[i], nullptr};
        ft.qpos[i] = ga.qpos[i] = qpos;
        ft.qvel[i] = ga.qvel[i] = qvel;
        ft.qt[i] = s.qt;
        ft.side[i] = bk.xside[i];
        StepInputs in = slot_inputs(s, wr);
        if (dv) { in.tgt = dv->tgt; in.tvel = dv->tvel; in.wrench = wr; }
        fill_params<T>(c, tr.p[i], B, in, dv ? dv->u : bk.u[i], dv ? dv->flags : bk.flags[i]);
        if (tp.prog == Program::LIST) {      // a tick of a slot with an action list: its own gains, which the action kernel writes per robot
            tr.p[i].gains = (const T*)s.prog.al_gains.get(); tr.p[i].null_kv = (const T*)s.prog.al_nullkv.get();
            tr.p[i].gains_per_instance = 1;
        }
        tr.x[i] = Row16Extra{c->dzeros, bk.list[i], bk.count + i, bk.xside[i], qvel, c->model.dtables, c->span_next};
        ga.out[i] = slot_out<T>(s);
        ga.list[i] = bk.list[i];
        ga.count[i] = bk.count + i;
    }
    // lane form of the OSC step: when every step of the train takes it (from_q_form) and the bank has its records
    bool use_lane = true;
    lane::LaneTrain lt;
    memset(&lt, 0, sizeof lt);
    for (int i = 0; i < n && use_lane; ++i) {
        const bool tvel = dv ? dv->tvel != nullptr : c->slot[slots[i]].has_tvel != 0;
        if (from_q_form(c, tvel) != FROMQ_LANE || !bk.lane_rec[i] || !bk.lane_count) use_lane = false;
        lt.qt[i] = c->slot[slots[i]].qt;
        lt.rec[i] = bk.lane_rec[i];
        lt.rec_count[i] = bk.lane_count + i;
    }
    if (use_lane) {
        lt.map = c->model.lane_map;
        HIPCHK(c, hipMemsetAsync(bk.lane_count, 0, R16_TRAIN * sizeof(int32_t), st));
    }
    if (c->tev_begin) HIPCHK(c, hipEventRecord(c->tev_begin, st));
    HIPCHK(c, (hipError_t)fused_walk(c).launch(c->model.dmodel, ft, n, st));
    int rcw = ft_launch(c, fts, nft, B, st);      // the sensor feed's wrench: read by every OSC kernel below (and the give-up pass)
    if (!rcw && pl) rcw = tick_front<T>(c, s0, B, tp, bk, nft ? fts[0].wrench : nullptr, st);
    if (rcw) return rcw;
    if (use_lane) HIPCHK(c, (hipError_t)launch_lane_osc<T>(tr, lt, n, c->model.lane_tier, lane_eig_blocks(), lane_eig_min(), st));
    else HIPCHK(c, (hipError_t)launch_row16_fromq<T>(tr, n, st));      // (task pass + FROMQ kernel; the lane kernel computes the task rows itself)
    HIPCHK(c, (hipError_t)launch_frontend_generic_lists<T>(c->model.dmodel, ga, n, c->model.fe_smem, st));
    HIPCHK(c, (hipError_t)launch_row16_worklist<T>(tr, n, nullptr, st));
    if (tp.reward) HIPCHK(c, (hipError_t)launch_reward<T>(reward_args(c, s0, B, s0.reward.d, s0.reward.per_robot, &bk, nft ? fts[0].wrench : nullptr), st));
    if (pl && pl->log) {      // the log's front launch; the first into a half of the ring that was draining waits for its copy
        if (pl->log->wait) HIPCHK(c, hipStreamWaitEvent(st, pl->log->wait, 0));
        HIPCHK(c, (hipError_t)launch_log<T>(log_args(c, s0, bk, *pl->log, LOG_FRONT, nft ? fts[0].wrench : nullptr), st));
    }
    if (pl && (rcw = tick_behind<T>(c, s0, B, tp, bk, *pl, st))) return rcw;
    if (c->tev_end) HIPCHK(c, hipEventRecord(c->tev_end, st));
    // The give-up pass wrote dense records of the robots on its lists into the slots (and nothing for the others): what the
    // slots held before no longer belongs to one state.  They hold no records from here on -- irlosc_step / irlosc_step_resident
    // / irlosc_download_records on them fail with IRLOSC_ERR_STATE until irlosc_frontend / irlosc_upload* fills them again.
    for (int i = 0; i < n; ++i) c->slot[slots[i]].voided();
    if (pl) tick_done(s0, B, tp);
    return IRLOSC_OK;
}
template <typename T>
static int fused_train_slots(irlosc_ctx* c, const int* slots, int n, int B, int k) {
    return fused_train<T>(c, slots, n, B, k, nullptr, c->plant_next);
}

// `iters` steps on the fused path.  Banks are allocated only when a call chains trains: one bank per train up to FQ_BANKS.
static int fused_resident(irlosc_ctx* c, int first_slot, int B, int iters) {
    const int ntrains = (iters + R16_TRAIN - 1) / R16_TRAIN;
    return run_trains(c, first_slot, B, iters, c->model.fq_overlap ? std::min((int)irlosc_ctx::FQ_BANKS, ntrains) : 1, fused_need(c), c->cfg.dtype == IRLOSC_F64 ? fused_train_slots<double> : fused_train_slots<float>);
}

// A step from the slot's coordinates through dense records: front end, the wrench of the slot's sensor feed (when it has one), step.
static int dense_from_q_step(irlosc_ctx* c, int slot, int B) {
    int rc = check_slot_q(c, slot, B);
    if (!rc) rc = check_slot_feed(c, slot, B);
    if (!rc) rc = frontend_launch(c, slot, B);
    void* wr = nullptr;
    if (!rc && c->slot[slot].feed > 0) {
        if (!(wr = feed_wrench(c, 0, 0))) return IRLOSC_ERR_HIP;
        const FtStep s{c->slot[slot].sens, wr, nullptr, c->slot[slot].ee};
        rc = ft_launch(c, &s, 1, B, c->stream);
    }
    if (!rc) rc = launch_slot(c, slot, B, wr);
    return rc;
}

extern "C" const char* irlosc_from_q_name(const irlosc_ctx* c) {
    static thread_local std::string nm;
    if (!c || !c->model.in_force) return "";
    const FromQ form = from_q_form(c, false);
    if (form == FROMQ_LANE) {
        char sh[64];
        const int* rows = lane::TIER_ROWS[c->model.lane_tier];
        snprintf(sh, sizeof sh, "osc_lane_%s_rows_%d_%d_%d + eigen pass", c->cfg.dtype == IRLOSC_F64 ? "f64" : "f32in_f64", rows[0], rows[1], rows[2]);
        nm = std::string(fused_walk(c).name) + " + " + sh +
             " (fused: compact exchange buffer, no dense M / J; OSC step one lane per robot; target velocities: " + c->kernel_name + "_fromq)";
    } else if (form == FROMQ_ROW16) nm = std::string(fused_walk(c).name) + " + " + c->kernel_name + "_fromq (fused: compact exchange buffer, no dense M / J)";
    else nm = std::string(irlosc_frontend_name(c)) + " + " + c->kernel_name + " (through dense records)";
    return nm.c_str();
}

extern "C" int irlosc_step_from_q(irlosc_ctx* c, int32_t slot, int32_t B, void* u_host, uint32_t* flags_host) {
    if (!c) return IRLOSC_ERR_ARG;
    int rc = check_slot(c, slot, B);
    if (rc) return rc;
    if (c->gains_nb == 0) return fail(c, IRLOSC_ERR_STATE, "irlosc_set_gains has not been called");
    HIPCHK(c, hipSetDevice(c->cfg.hip_device));
    if (B > 0) {
        rc = fused_ready(c, 1) ? fused_resident(c, slot, B, 1) : dense_from_q_step(c, slot, B);
        if (rc) return rc;
    }
    if (u_host || flags_host) return irlosc_download(c, B, u_host, flags_host);
    return IRLOSC_OK;
}

extern "C" int irlosc_step_resident_from_q(irlosc_ctx* c, int32_t first_slot, int32_t B, int32_t iters, float* ms_total,
                                           float* ms_step_avg) {
    return timed_resident(c, first_slot, B, iters, ms_total, ms_step_avg, [&] {
        if (B > 0 && fused_ready(c, std::min((int)R16_TRAIN, iters))) return fused_resident(c, first_slot, B, iters);
        int rc = IRLOSC_OK;
        for (int i = 0; i < iters && !rc; ++i) rc = dense_from_q_step(c, (first_slot + i) % c->cfg.n_slots, B);
        return rc;
    });
}

// ---- F/T sensor feed of the steps from joint coordinates ------------------------------------------------------------
static void mat_mul(const double* A, const double* B, double* C, bool at = false) {     // C = A B (at: A^T B)
    double t[9];
    for (int r = 0; r < 3; ++r)
        for (int cc = 0; cc < 3; ++cc) {
            double v = 0;
            for (int i = 0; i < 3; ++i) v += (at ? A[i * 3 + r] : A[r * 3 + i]) * B[i * 3 + cc];
            t[r * 3 + cc] = v;
        }
    memcpy(C, t, sizeof t);
}

extern "C" int irlosc_set_ft_sensors(irlosc_ctx* c, const irlosc_ft_desc* fd) {
    if (!c) return IRLOSC_ERR_ARG;
    if (!fd) return fail(c, IRLOSC_ERR_ARG, "desc is NULL");
    if (!c->model.in_force) return fail(c, IRLOSC_ERR_STATE, "irlosc_set_model has not been called");
    const FeModel& h = c->model.h;
    const int32_t* par = h.parent;
    int32_t f0[IRLOSC_MAX_DEV], t0[IRLOSC_MAX_DEV];
    double R[IRLOSC_MAX_DEV][9];
    for (int d = 0; d < c->cfg.ndev; ++d) {
        f0[d] = t0[d] = -1;
        for (int i = 0; i < 9; ++i) R[d][i] = (i % 4 == 0) ? 1.0 : 0.0;
        const int sb = fd->site_body[d], e = h.ee_body[d];
        if (sb < 0) continue;
        if (sb >= h.nb) return fail(c, IRLOSC_ERR_ARG, "device %d: site_body %d out of [0,%d)", d, sb, h.nb);
        if (fd->n_sensor < 3) return fail(c, IRLOSC_ERR_ARG, "device %d: n_sensor=%d holds no triple", d, fd->n_sensor);
        if (fd->ft_force0[d] < 0 || fd->ft_force0[d] > fd->n_sensor - 3 || fd->ft_torque0[d] < 0 || fd->ft_torque0[d] > fd->n_sensor - 3)
            return fail(c, IRLOSC_ERR_ARG, "device %d: sensordata indices force %d / torque %d out of [0,%d]", d, fd->ft_force0[d],
                        fd->ft_torque0[d], fd->n_sensor - 3);
        // the tree path between the site body and the EE body runs through their deepest common ancestor `a` (-1: the world); every
        // body on it below `a` must be welded to its parent
        auto above = [&](int x, int y) { for (int z = y; z >= 0; z = par[z]) if (z == x) return true; return x < 0; };   // x ancestor-or-self of y
        int a = e;
        while (a >= 0 && !above(a, sb)) a = par[a];
        double P[2][9];
        const int ends[2] = {sb, e};
        for (int s = 0; s < 2; ++s) {
            for (int i = 0; i < 9; ++i) P[s][i] = (i % 4 == 0) ? 1.0 : 0.0;
            for (int x = ends[s]; x != a; x = par[x]) {      // P = R(q_x) P, from `ends[s]` up: P = R(child of a) ... R(ends[s])
                if (h.joint_of_body[x] >= 0)
                    return fail(c, IRLOSC_ERR_ARG, "device %d: the F/T site body %d is not rigidly attached to the EE body %d (hinge %d of body %d "
                                "lies between them)", d, sb, e, h.joint_of_body[x], x);
                double Rx[9];
                quat_mat(h.quat[x], Rx, true);
                mat_mul(Rx, P[s], P[s]);
            }
        }
        double Rs[9];
        quat_mat(fd->site_quat[d], Rs, true);
        mat_mul(P[0], Rs, P[0]);                   // R(a)^T R(site) = P_site R(site_quat)
        mat_mul(P[1], P[0], R[d], true);           // R_rel = R(ee)^T R(site) = P_ee^T P_site R(site_quat)
        f0[d] = fd->ft_force0[d]; t0[d] = fd->ft_torque0[d];
    }
    for (int d = 0; d < c->cfg.ndev; ++d) {
        c->ft_f0[d] = f0[d]; c->ft_t0[d] = t0[d];
        for (int i = 0; i < 9; ++i) c->ft_R[d][i] = R[d][i];
    }
    c->ft_n_sensor = fd->n_sensor;
    c->ft_set = 1;
    for (Slot& s : c->slot) s.end_feed();      // feeds laid out for another description
    return IRLOSC_OK;
}

extern "C" int irlosc_set_sensordata(irlosc_ctx* c, int32_t slot, int32_t B, const double* sensordata) {
    if (!c) return IRLOSC_ERR_ARG;
    int rc = check_slot(c, slot, B);
    if (rc) return rc;
    Slot& s = c->slot[slot];
    if (B == 0 || !sensordata) { s.end_feed(); return IRLOSC_OK; }
    if (!c->ft_set) return fail(c, IRLOSC_ERR_STATE, "irlosc_set_ft_sensors has not been called");
    HIPCHK(c, hipSetDevice(c->cfg.hip_device));
    const size_t Bm = (size_t)c->cfg.max_batch, ns = (size_t)c->ft_n_sensor;
    s.end_feed();      // (none until the new one is in the buffer)
    HIPCHK(c, s.sens.reserve(Bm * ns * sizeof(double)));
    HIPCHK(c, hipMemcpyAsync(s.sens, sensordata, (size_t)B * ns * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    s.feed = B;
    return IRLOSC_OK;
}

extern "C" int irlosc_step_from_q_device(irlosc_ctx* c, int32_t slot, int32_t B, const double* d_qpos, const double* d_qvel,
                                         const void* d_tgt_pose, const void* d_tgt_vel, const double* d_sensordata,
                                         void* d_u, uint32_t* d_flags, void* hip_stream) {
    if (!c) return IRLOSC_ERR_ARG;
    int rc = check_slot(c, slot, B);
    if (rc) return rc;
    if (B == 0) return IRLOSC_OK;
    if (!d_qpos || !d_qvel || !d_tgt_pose || !d_u || !d_flags) return fail(c, IRLOSC_ERR_ARG, "d_qpos, d_qvel, d_tgt_pose, d_u and d_flags are required");
    if (!c->model.in_force) return fail(c, IRLOSC_ERR_STATE, "irlosc_set_model has not been called");
    if (c->gains_nb == 0) return fail(c, IRLOSC_ERR_STATE, "irlosc_set_gains has not been called");
    if (d_sensordata && !c->ft_set) return fail(c, IRLOSC_ERR_STATE, "d_sensordata given but irlosc_set_ft_sensors has not been called");
    HIPCHK(c, hipSetDevice(c->cfg.hip_device));
    const hipStream_t st = hip_stream ? (hipStream_t)hip_stream : c->stream;
    const bool fused = fused_ready(c, 1);      // (first call: allocates bank 0's exchange buffer / lane records on the context's stream)
    Slot& s = c->slot[slot];
    if (fused) HIPCHK(c, s.qt.ensure(qt_bytes(c)));
    if (st != c->stream) {                     // ... and whatever else the context's stream holds comes first
        HIPCHK(c, c->ev_dev.ensure(hipEventDisableTiming));
        HIPCHK(c, hipEventRecord(c->ev_dev, c->stream));
        HIPCHK(c, hipStreamWaitEvent(st, c->ev_dev, 0));
    }
    s.lent(d_sensordata != nullptr);      // from here on the slot's records and coordinates are scratch of this call
    const DevCall dv{d_qpos, d_qvel, d_tgt_pose, d_tgt_vel, d_sensordata, d_u, d_flags, st};
    if (fused) {
        HIPCHK(c, (hipError_t)launch_q_layout(d_qpos, d_qvel, s.qt, B, c->cfg.n, st));
        const int sl = slot;
        rc = c->cfg.dtype == IRLOSC_F64 ? fused_train<double>(c, &sl, 1, B, 0, &dv) : fused_train<float>(c, &sl, 1, B, 0, &dv);
    } else {
        rc = frontend_launch(c, slot, B, d_qpos, d_qvel, st);
        if (!rc && d_sensordata) {
            const FtStep fs{d_sensordata, s.wrench, nullptr, s.ee};
            rc = ft_launch(c, &fs, 1, B, st);
        }
        StepInputs in = slot_inputs(s);
        in.tgt = d_tgt_pose; in.tvel = d_tgt_vel; in.wrench = d_sensordata ? s.wrench : nullptr;
        if (!rc) rc = launch(c, B, in, d_u, d_flags, st, row16_route(record_route(c, slot, B)) == IRLOSC_ROUTE_ROW16_TREE);
    }
    s.lent(d_sensordata != nullptr);      // (the front end / fused_train mark what they wrote: none of it is the slot's state)
    return rc;
}

// ---- closed loops on the GPU: the plant behind the fused step (osc_plant.hpp) ---------------------------------------------
extern "C" int irlosc_set_plant(irlosc_ctx* c, const irlosc_plant* p) {
    if (!c) return IRLOSC_ERR_ARG;
    if (!p) return fail(c, IRLOSC_ERR_ARG, "plant is NULL");
    if (!c->model.in_force) return fail(c, IRLOSC_ERR_STATE, "irlosc_set_model has not been called");
    if (!(std::isfinite(p->dt) && p->dt > 0.0)) return fail(c, IRLOSC_ERR_ARG, "plant: dt=%g must be finite and > 0", p->dt);
    if (!(std::isfinite(p->damping) && p->damping >= 0.0)) return fail(c, IRLOSC_ERR_ARG, "plant: damping=%g must be finite and >= 0", p->damping);
    if (p->reserved != 0) return fail(c, IRLOSC_ERR_ARG, "plant: reserved must be 0");
    if (c->cfg.n < 32 && (p->ctrl_mask >> c->cfg.n)) return fail(c, IRLOSC_ERR_ARG, "plant: ctrl_mask has bits >= n=%d", c->cfg.n);
    c->plant = *p;
    c->plant_set = 1;
    return IRLOSC_OK;
}

extern "C" int irlosc_download_q(irlosc_ctx* c, int32_t slot, int32_t B, double* qpos, double* qvel) {
    if (!c) return IRLOSC_ERR_ARG;
    int rc = check_slot(c, slot, B);
    if (rc) return rc;
    const Slot& s = c->slot[slot];
    if (B > std::max(0, s.coords)) return fail(c, IRLOSC_ERR_STATE, "slot %d holds joint coordinates of %d instances", slot, std::max(0, s.coords));
    if (B == 0) return IRLOSC_OK;
    HIPCHK(c, hipSetDevice(c->cfg.hip_device));
    const size_t bytes = (size_t)B * c->cfg.n * sizeof(double);
    if (qpos) HIPCHK(c, hipMemcpyAsync(qpos, s.qpos, bytes, hipMemcpyDeviceToHost, c->stream));
    if (qvel) HIPCHK(c, hipMemcpyAsync(qvel, s.qvel, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return IRLOSC_OK;
}

// The episode log of one call of irlosc_rollout_from_q_logged: what every logged tick's LogCall shares, where the samples go on the host, the
// ring's shape (two halves of `hcap` samples of `words` doubles), and per half what is on its way: samples first .. first + count - 1 in
// the half's pinned block behind its `drained` event (count 0: nothing), and whether the half has been drained before in this call
struct LogRun {
    LogCall call{};
    int every = 1, nsamples = 0, hcap = 1;
    size_t words = 0;
    double* host = nullptr;
    struct { int first = 0, count = 0; bool drained = false; } half[2];
};

// The samples of half h that are on their way arrive in log_host: the host waits for the half's copy (keep: and copies the pinned block on)
static int log_collect(irlosc_ctx* c, LogRun& lr, int h, bool keep = true) {
    if (!lr.half[h].count) return IRLOSC_OK;
    const int first = lr.half[h].first, count = lr.half[h].count;
    lr.half[h].count = 0;
    HIPCHK(c, hipEventSynchronize(c->log_drained[h]));
    if (keep) memcpy(lr.host + (size_t)first * lr.words, (const unsigned char*)c->log_stage[h], (size_t)count * lr.words * sizeof(double));
    return IRLOSC_OK;
}

// Half h holds samples first .. first + count - 1: they leave on log_stream behind the ticks that wrote them, into the half's pinned block
// (which the host empties first if its last load is still there), while the rollout's stream goes on into the other half
static int log_drain(irlosc_ctx* c, LogRun& lr, int h, int first, int count) {
    HIPCHK(c, hipEventRecord(c->log_full[h], c->stream));
    const int rc = log_collect(c, lr, h);
    if (rc) return rc;
    HIPCHK(c, hipStreamWaitEvent(c->log_stream, c->log_full[h], 0));
    HIPCHK(c, hipMemcpyAsync((unsigned char*)c->log_stage[h], c->dlog + (size_t)h * lr.hcap * lr.words, (size_t)count * lr.words * sizeof(double),
                             hipMemcpyDeviceToHost, c->log_stream));
    HIPCHK(c, hipEventRecord(c->log_drained[h], c->log_stream));
    lr.half[h].first = first; lr.half[h].count = count; lr.half[h].drained = true;
    return IRLOSC_OK;
}

// The end of a logged call, error or not: both halves arrive (rc != 0: are waited for and dropped) and log_stream is joined -> rc, or the
// first error here.  The caller joins the rollout's stream.
static int log_join(irlosc_ctx* c, LogRun& lr, int rc) {
    const int older = lr.half[0].count && lr.half[1].count && lr.half[1].first < lr.half[0].first ? 1 : 0;
    for (int i = 0; i < 2; ++i) {
        const int e = log_collect(c, lr, i ? 1 - older : older, rc == IRLOSC_OK);
        if (e && !rc) rc = e;
    }
    const hipError_t es = hipStreamSynchronize(c->log_stream);
    if (es != hipSuccess && !rc) rc = fail(c, IRLOSC_ERR_HIP, "hipStreamSynchronize of the log's stream failed: %s", hipGetErrorString(es));
    return rc;
}

// The ticks of a rollout, enqueued; the caller synchronises (also after an error: earlier ticks are in flight) and, with a log, joins it
// (log_join).  One frame for the unlogged and the logged entry point: lr == nullptr is the rollout without a log.
static int rollout_ticks(irlosc_ctx* c, int slot, int B, int ticks, int every, double* trace_host, LogRun* lr = nullptr) {
    const size_t sample = (size_t)B * c->cfg.ndev * 7;      // doubles
    const int nsamples = every > 0 && trace_host ? (ticks + every - 1) / every : 0;
    // the trace's device buffer: whole samples up to TRACE_BYTES, at least one; a chunk goes to the host when it is full
    constexpr size_t TRACE_BYTES = (size_t)256 << 20;
    const size_t max_sample = (size_t)c->cfg.max_batch * c->cfg.ndev * 7 * sizeof(double);
    const int cap = (int)std::max<size_t>(1, TRACE_BYTES / max_sample);
    if (nsamples && !got(c->dtrace.ensure((size_t)cap * max_sample)))
        return fail(c, IRLOSC_ERR_HIP, "out of device memory for the EE trace (%zu bytes)", (size_t)cap * max_sample);
    HIPCHK(c, hipMemsetAsync(c->dflags_any, 0, (size_t)B * sizeof(uint32_t), c->stream));
    int filled = 0, sent = 0;      // samples written / copied to the host
    int logged_n = 0;              // samples of the log written
    // The early exit of a slot with episodes (include/irlosc.h: its formula): after the ticks P - 1, 2 P - 1, ... the waves' running counts
    // go to one of two pinned blocks behind an event; before tick m P (m >= 2) the host waits for the copy made after tick (m - 1) P - 1
    // and stops there if no robot of the call is running.  Waiting makes the ticks run a function of the inputs.  P == 0: none of it.
    Slot& s0 = c->slot[slot];
    const int P = s0.episodes.robots ? s0.episodes.d.poll_every : 0, waves = (B + 63) / 64;
    int32_t* const run_host = (int32_t*)(unsigned char*)c->run_stage;
    int t = 0;
    for (; t < ticks; ++t) {
        if (P && t % P == 0 && t >= 2 * P) {
            const int h = (t / P - 1) % 2;
            HIPCHK(c, hipEventSynchronize(c->run_copied[h]));
            int running = 0;
            for (int w = 0; w < waves; ++w) running += run_host[(size_t)h * waves + w];
            if (!running) break;
        }
        const bool traced = nsamples && t % every == 0;
        const bool logged = lr && t % lr->every == 0;
        const int lh = logged ? (logged_n / lr->hcap) % 2 : 0, lpos = logged ? logged_n % lr->hcap : 0;      // the log's half and place in it
        if (logged) {
            lr->call.sample = c->dlog + ((size_t)lh * lr->hcap + lpos) * lr->words;
            lr->call.wait = lpos == 0 && lr->half[lh].drained ? (hipEvent_t)c->log_drained[lh] : nullptr;
        }
        const PlantCall pl{traced ? c->dtrace + (size_t)(filled % cap) * sample : nullptr, logged ? &lr->call : nullptr};
        c->plant_next = &pl;
        const int rc = fused_resident(c, slot, B, 1);
        c->plant_next = nullptr;
        if (rc) return rc;
        if (logged && (++logged_n % lr->hcap == 0 || logged_n == lr->nsamples)) {      // the half is full, or holds the last sample
            const int rcl = log_drain(c, *lr, lh, logged_n - 1 - lpos, lpos + 1);
            if (rcl) return rcl;
        }
        if (traced && (++filled % cap == 0 || filled == nsamples)) {
            HIPCHK(c, hipMemcpyAsync(trace_host + (size_t)sent * sample, c->dtrace, (size_t)(filled - sent) * sample * sizeof(double),
                                     hipMemcpyDeviceToHost, c->stream));
            sent = filled;
        }
        if (P && (t + 1) % P == 0 && t + 1 + P < ticks) {      // (a copy nobody would wait for is not made)
            const int h = ((t + 1) / P) % 2;
            HIPCHK(c, hipMemcpyAsync(run_host + (size_t)h * waves, s0.episodes.running, (size_t)waves * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipEventRecord(c->run_copied[h], c->stream));
        }
    }
    s0.ticks_run = t;
    if (t < ticks) {      // an early exit: what the ticks run have written and not yet sent leaves now
        if (lr && logged_n % lr->hcap != 0 && logged_n != lr->nsamples) {
            const int n = logged_n % lr->hcap, rcl = log_drain(c, *lr, ((logged_n - 1) / lr->hcap) % 2, logged_n - n, n);
            if (rcl) return rcl;
        }
        if (filled > sent)
            HIPCHK(c, hipMemcpyAsync(trace_host + (size_t)sent * sample, c->dtrace, (size_t)(filled - sent) * sample * sizeof(double),
                                     hipMemcpyDeviceToHost, c->stream));
    }
    return IRLOSC_OK;
}

extern "C" int irlosc_log_layout_reward(int32_t n, int32_t ndev, int32_t nobj, int32_t n_out, int32_t sampled, int32_t rewarded, uint32_t channels, int32_t R,
                                        int64_t offset[13], int64_t* sample_words) {
    if (!offset || !sample_words) return fail(nullptr, IRLOSC_ERR_ARG, "log: offset and sample_words are required");
    if (nobj < 0 || nobj > IRLOSC_MAX_OBJECTS) return fail(nullptr, IRLOSC_ERR_ARG, "log: nobj=%d out of [0,%d]", nobj, IRLOSC_MAX_OBJECTS);
    if (n_out != 0 && n_out != 6 && n_out != 7) return fail(nullptr, IRLOSC_ERR_ARG, "log: n_out=%d must be 0 (no policy), 6 or 7", n_out);
    if (sampled != 0 && sampled != 1) return fail(nullptr, IRLOSC_ERR_ARG, "log: sampled=%d must be 0 or 1", sampled);
    if (rewarded != 0 && rewarded != 1) return fail(nullptr, IRLOSC_ERR_ARG, "log: rewarded=%d must be 0 or 1", rewarded);
    const uint32_t known = (LOG_FRONT | LOG_BACK) & ~(nobj ? 0u : (uint32_t)IRLOSC_LOG_OBJECT_POSE)      // (no objects, no policy, no head, no reward: no such channel)
                           & ~(n_out ? 0u : (uint32_t)IRLOSC_LOG_POLICY_OUT) & ~(n_out && sampled ? 0u : (uint32_t)IRLOSC_LOG_POLICY_SAMPLE)
                           & ~(rewarded ? 0u : (uint32_t)IRLOSC_LOG_REWARD);
    if (channels == 0 || (channels & ~known)) return fail(nullptr, IRLOSC_ERR_ARG, "log: channels=0x%x must be a non-empty OR of the IRLOSC_LOG_* bits", channels);
    if (R < 1) return fail(nullptr, IRLOSC_ERR_ARG, "log: R=%d must be >= 1", R);
    if (n < 1 || n > IRLOSC_MAX_N) return fail(nullptr, IRLOSC_ERR_ARG, "log: n=%d out of [1,%d]", n, IRLOSC_MAX_N);
    if (ndev < 1 || ndev > IRLOSC_MAX_DEV) return fail(nullptr, IRLOSC_ERR_ARG, "log: ndev=%d out of [1,%d]", ndev, IRLOSC_MAX_DEV);
    int64_t words = 0;
    for (int i = 0; i < LOG_CHANNELS; ++i) {
        offset[i] = (channels >> i) & 1u ? words : -1;
        if ((channels >> i) & 1u) words += (int64_t)R * log_width(i, n, ndev, nobj, n_out);
    }
    *sample_words = words;
    return IRLOSC_OK;
}

extern "C" int irlosc_log_layout_policy(int32_t n, int32_t ndev, int32_t nobj, int32_t n_out, int32_t sampled, uint32_t channels, int32_t R, int64_t offset[12],
                                        int64_t* sample_words) {
    int64_t off[LOG_CHANNELS];
    const int rc = irlosc_log_layout_reward(n, ndev, nobj, n_out, sampled, 0, channels, R, offset ? off : nullptr, sample_words);
    for (int i = 0; !rc && i < 12; ++i) offset[i] = off[i];
    return rc;
}

extern "C" int irlosc_log_layout_objects(int32_t n, int32_t ndev, int32_t nobj, uint32_t channels, int32_t R, int64_t offset[10], int64_t* sample_words) {
    int64_t off[LOG_CHANNELS];
    const int rc = irlosc_log_layout_policy(n, ndev, nobj, 0, 0, channels, R, offset ? off : nullptr, sample_words);
    for (int i = 0; !rc && i < 10; ++i) offset[i] = off[i];
    return rc;
}

extern "C" int irlosc_log_layout(int32_t n, int32_t ndev, uint32_t channels, int32_t R, int64_t offset[9], int64_t* sample_words) {
    int64_t off[LOG_CHANNELS];
    const int rc = irlosc_log_layout_objects(n, ndev, 0, channels, R, offset ? off : nullptr, sample_words);
    for (int i = 0; !rc && i < 9; ++i) offset[i] = off[i];
    return rc;
}

// The log of a call, checked against the slot (every refusal ahead of the first allocation or launch) and planned into lr; B >= 1
static int log_plan(irlosc_ctx* c, int slot, int B, int ticks, const irlosc_log* log, const int32_t* robots, double* log_host, LogRun& lr) {
    if (log->every < 1) return fail(c, IRLOSC_ERR_ARG, "log: every=%d must be >= 1", log->every);
    if (log->reserved != 0) return fail(c, IRLOSC_ERR_ARG, "log: reserved must be 0");
    if (!log_host) return fail(c, IRLOSC_ERR_ARG, "log: log_host is NULL");
    if (!robots && log->n_robots != 0 && log->n_robots != B)
        return fail(c, IRLOSC_ERR_ARG, "log: n_robots=%d without robots[] must be 0 or B=%d", log->n_robots, B);
    if (robots && (log->n_robots < 1 || log->n_robots > B)) return fail(c, IRLOSC_ERR_ARG, "log: n_robots=%d out of [1,%d]", log->n_robots, B);
    const int R = robots ? log->n_robots : B;
    for (int i = 0; robots && i < R; ++i)
        if (robots[i] < 0 || robots[i] >= B || (i && robots[i] <= robots[i - 1]))
            return fail(c, IRLOSC_ERR_ARG, "log: robots[%d]=%d: the list must be strictly ascending in [0,%d)", i, robots[i], B);
    int64_t words = 0;
    const Program& pg = c->slot[slot].prog;      // (a policy's channels: POLICY_OUT with a policy, POLICY_SAMPLE with its Gaussian head)
    if (irlosc_log_layout_reward(c->cfg.n, c->cfg.ndev, c->slot[slot].objects.count(), pg.kind == Program::POLICY ? pg.po.n_out : 0, pg.noise, c->slot[slot].reward.robots ? 1 : 0, log->channels, R,
                                 lr.call.off, &words))
        return fail(c, IRLOSC_ERR_ARG, "%s", irlosc_last_error(nullptr));
    const uint64_t sb = (uint64_t)words * sizeof(double);      // (R <= max_batch, 170 words a robot at most: far from 2^63)
    if (log->buffer_bytes && log->buffer_bytes / 2 < sb)
        return fail(c, IRLOSC_ERR_ARG, "log: buffer_bytes=%llu holds fewer than two samples of %llu bytes", (unsigned long long)log->buffer_bytes, (unsigned long long)sb);
    const Slot& s = c->slot[slot];
    if ((log->channels & IRLOSC_LOG_WRENCH) && s.feed <= 0) return fail(c, IRLOSC_ERR_STATE, "log: IRLOSC_LOG_WRENCH on slot %d, which has no sensor feed (irlosc_set_sensordata)", slot);
    if ((log->channels & IRLOSC_LOG_WALL_FORCE) && !s.walls.robots) return fail(c, IRLOSC_ERR_STATE, "log: IRLOSC_LOG_WALL_FORCE on slot %d, which has no walls (irlosc_set_walls)", slot);
    if ((log->channels & IRLOSC_LOG_JOINT_TAU) && !s.joints.robots) return fail(c, IRLOSC_ERR_STATE, "log: IRLOSC_LOG_JOINT_TAU on slot %d, which has no joint rows (irlosc_set_joints)", slot);
    // the ring: two halves of whole samples; a half holds what drains in one piece (DRAIN_BYTES, or one sample where that is larger: short
    // pieces keep the last one, which nothing overlaps, short), never more than the ring's half or the call's samples
    constexpr uint64_t RING_BYTES = (uint64_t)256 << 20, DRAIN_BYTES = (uint64_t)32 << 20;
    const uint64_t ring = log->buffer_bytes ? log->buffer_bytes : std::max(RING_BYTES, 2 * sb);
    lr.every = log->every;
    lr.nsamples = (ticks + log->every - 1) / log->every;
    lr.hcap = (int)std::min<uint64_t>(std::min(ring / 2 / sb, std::max<uint64_t>(1, DRAIN_BYTES / sb)), (uint64_t)lr.nsamples);
    lr.words = (size_t)words;
    lr.host = log_host;
    lr.call.channels = log->channels; lr.call.R = R;
    return IRLOSC_OK;
}

// The log's buffers for the call lr plans: ring, pinned blocks, stream and events (each made by the first use, grown on demand), and the
// index list on the device
static int log_buffers(irlosc_ctx* c, const int32_t* robots, LogRun& lr) {
    const size_t half = (size_t)lr.hcap * lr.words * sizeof(double);
    if (!got(c->dlog.reserve(2 * half))) return fail(c, IRLOSC_ERR_HIP, "out of device memory for the log's ring (%zu bytes)", 2 * half);
    for (int h = 0; h < (lr.nsamples > lr.hcap ? 2 : 1); ++h)
        if (!got(c->log_stage[h].reserve(half))) return fail(c, IRLOSC_ERR_HIP, "out of pinned host memory for the log (%zu bytes)", half);
    HIPCHK(c, c->log_stream.ensure());
    for (int h = 0; h < 2; ++h) {
        HIPCHK(c, c->log_full[h].ensure(hipEventDisableTiming));
        HIPCHK(c, c->log_drained[h].ensure(hipEventDisableTiming));
    }
    if (robots) {
        if (!got(c->dlog_robots.reserve((size_t)c->cfg.max_batch * sizeof(int32_t)))) return fail(c, IRLOSC_ERR_HIP, "out of device memory for the log's robot list");
        HIPCHK(c, hipMemcpyAsync(c->dlog_robots, robots, (size_t)lr.call.R * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
        lr.call.robots = c->dlog_robots;
    }
    return IRLOSC_OK;
}

// Both rollout entry points: the EE trace (irlosc_rollout_from_q) or the episode log (irlosc_rollout_from_q_logged), or neither
static int rollout_call(irlosc_ctx* c, int32_t slot, int32_t B, int32_t ticks, int32_t trace_every, double* ee_trace_host, const irlosc_log* log,
                        const int32_t* robots, double* log_host, void* u_host, uint32_t* flags_any_host) {
    if (!c) return IRLOSC_ERR_ARG;
    int rc = check_slot(c, slot, B);
    if (rc) return rc;
    if (ticks < 1) return fail(c, IRLOSC_ERR_ARG, "ticks=%d must be >= 1", ticks);
    if (trace_every < 0) return fail(c, IRLOSC_ERR_ARG, "trace_every=%d must be >= 0", trace_every);
    if (!c->model.in_force) return fail(c, IRLOSC_ERR_STATE, "irlosc_set_model has not been called");
    if (!c->plant_set) return fail(c, IRLOSC_ERR_STATE, "irlosc_set_plant has not been called (since the last irlosc_set_model)");
    if (c->gains_nb == 0) return fail(c, IRLOSC_ERR_STATE, "irlosc_set_gains has not been called");
    if (!c->model.fused)
        return fail(c, IRLOSC_ERR_STATE, "no rollout on this context: the plant reads the exchange buffer of the fused path, which is off (%s); "
                    "steps from joint coordinates run %s", env_off("IRLOSC_FUSED") ? "IRLOSC_FUSED=0" :
                    c->kernel != IRLOSC_KERNEL_ROW16 ? "the context runs the generic kernel" : c->model.fe_lane ? "its buffers could not be allocated"
                    : "the model has not the compiled Dual-UR5 tree, or IRLOSC_FRONTEND=generic", irlosc_from_q_name(c));
    if (c->cfg.n != plant_joints()) return fail(c, IRLOSC_ERR_STATE, "no rollout on this context: the plant kernel holds %d joints, n=%d", plant_joints(), c->cfg.n);
    rc = check_slot_q(c, slot, B);
    if (!rc) rc = check_slot_feed(c, slot, B);
    if (!rc) rc = check_program(c, slot, B);
    if (!rc) rc = check_policy_objects(c, slot, B);
    if (!rc) rc = check_covers(c, slot, B, c->slot[slot].push.robots, "pushes", "cover", nullptr);
    if (!rc) rc = check_covers(c, slot, B, c->slot[slot].walls.robots, "walls", "cover", nullptr);
    if (!rc) rc = check_covers(c, slot, B, c->slot[slot].joints.robots, "joint rows", "cover", nullptr);
    if (!rc) rc = check_covers(c, slot, B, c->slot[slot].objects.robots, "action objects", "cover", nullptr);
    if (!rc) rc = check_covers(c, slot, B, c->slot[slot].loads.robots, "object loads", "cover", nullptr);
    if (!rc) rc = check_covers(c, slot, B, c->slot[slot].reward.robots, "reward", "covers", nullptr);
    if (!rc && c->slot[slot].reward.robots) rc = check_reward_refs(c, slot, B, c->slot[slot].reward.d);
    if (!rc) rc = check_covers(c, slot, B, c->slot[slot].episodes.robots, "episodes", "cover", nullptr);
    if (rc) return rc;
    c->slot[slot].ticks_run = B == 0 ? ticks : 0;      // (rollout_ticks says how many were enqueued; an empty batch: all, none of them a launch)
    if (B == 0) return IRLOSC_OK;
    LogRun lr;
    if (log && (rc = log_plan(c, slot, B, ticks, log, robots, log_host, lr))) return rc;
    HIPCHK(c, hipSetDevice(c->cfg.hip_device));
    if (!fused_ready(c, 1))
        return fail(c, IRLOSC_ERR_STATE, "no rollout on this context: the exchange buffers of the fused path could not be allocated (the path "
                    "is switched off; steps from joint coordinates run through dense records)");
    HIPCHK(c, c->slot[slot].qt.ensure(qt_bytes(c)));
    if (!got(c->dflags_any.ensure((size_t)c->cfg.max_batch * sizeof(uint32_t)))) return fail(c, IRLOSC_ERR_HIP, "out of device memory for flags_any");
    if (c->slot[slot].episodes.robots && c->slot[slot].episodes.d.poll_every) {      // the early exit's pinned blocks and events
        if (!got(c->run_stage.reserve(2 * (((size_t)c->cfg.max_batch + 63) / 64) * sizeof(int32_t))))
            return fail(c, IRLOSC_ERR_HIP, "out of pinned host memory for the early exit");
        for (int h = 0; h < 2; ++h) HIPCHK(c, c->run_copied[h].ensure(hipEventDisableTiming));
    }
    // (from here on work may be in flight: every path below joins the streams before it returns)
    if (log) rc = log_buffers(c, robots, lr);
    if (!rc) rc = rollout_ticks(c, slot, B, ticks, trace_every, ee_trace_host, log ? &lr : nullptr);
    if (log && c->log_stream) rc = log_join(c, lr, rc);
    if (!rc && u_host) {
        const hipError_t e = hipMemcpyAsync(u_host, c->du, (size_t)B * c->cfg.n * c->esz, hipMemcpyDeviceToHost, c->stream);
        if (e != hipSuccess) rc = fail(c, IRLOSC_ERR_HIP, "copy of u failed: %s", hipGetErrorString(e));
    }
    if (!rc && flags_any_host) {
        const hipError_t e = hipMemcpyAsync(flags_any_host, c->dflags_any, (size_t)B * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream);
        if (e != hipSuccess) rc = fail(c, IRLOSC_ERR_HIP, "copy of flags_any failed: %s", hipGetErrorString(e));
    }
    const hipError_t es = hipStreamSynchronize(c->stream);
    if (es != hipSuccess && !rc) rc = fail(c, IRLOSC_ERR_HIP, "hipStreamSynchronize failed: %s", hipGetErrorString(es));
    return rc;
}

extern "C" int irlosc_rollout_from_q(irlosc_ctx* c, int32_t slot, int32_t B, int32_t ticks, int32_t trace_every, double* ee_trace_host,
                                     void* u_host, uint32_t* flags_any_host) {
    return rollout_call(c, slot, B, ticks, trace_every, ee_trace_host, nullptr, nullptr, nullptr, u_host, flags_any_host);
}

extern "C" int irlosc_rollout_from_q_logged(irlosc_ctx* c, int32_t slot, int32_t B, int32_t ticks, const irlosc_log* log, const int32_t* robots,
                                            double* log_host, void* u_host, uint32_t* flags_any_host) {
    return rollout_call(c, slot, B, ticks, 0, nullptr, log, robots, log_host, u_host, flags_any_host);
}

// ---- waypoint paths of the rollout (osc_waypoint.hpp) -----------------------------------------------------------------------
extern "C" int irlosc_set_waypoints(irlosc_ctx* c, int32_t slot, int32_t B, const irlosc_waypoints* w, const double* xyz) {
    if (!c) return IRLOSC_ERR_ARG;
    int rc = check_slot(c, slot, B);
    if (rc) return rc;
    if (!c->model.in_force) return fail(c, IRLOSC_ERR_STATE, "irlosc_set_model has not been called");
    Slot& s = c->slot[slot];
    const int nd = c->cfg.ndev;
    int wmax = 0;
    for (int d = 0; w && d < IRLOSC_MAX_DEV; ++d) {
        if (w->count[d] < 0 || w->count[d] > IRLOSC_MAX_WAYPOINTS || (d >= nd && w->count[d] != 0))
            return fail(c, IRLOSC_ERR_ARG, "waypoints: count[%d]=%d out of [0,%d]", d, w->count[d], d < nd ? IRLOSC_MAX_WAYPOINTS : 0);
        wmax = std::max(wmax, (int)w->count[d]);
    }
    if (!w || wmax == 0) { if (s.prog.kind == Program::PATHS) s.episodes.end(); s.prog.end(Program::PATHS); return IRLOSC_OK; }
    if (B < 1) return fail(c, IRLOSC_ERR_ARG, "waypoints: B=%d must be >= 1", B);
    if (w->nb != 1 && w->nb != B) return fail(c, IRLOSC_ERR_ARG, "waypoints: nb=%d must be 1 or B=%d", w->nb, B);
    if (!xyz) return fail(c, IRLOSC_ERR_ARG, "waypoints: xyz is NULL");
    // the table as given, but for entries no device lists: zero whatever the caller's array holds there
    const size_t E = (size_t)nd * wmax * 3;
    std::vector<double> dense((size_t)w->nb * E, 0.0);
    for (int d = 0; d < nd; ++d) {
        if (!w->count[d]) continue;
        if (!(std::isfinite(w->threshold[d]) && w->threshold[d] > 0.0))
            return fail(c, IRLOSC_ERR_ARG, "waypoints: threshold[%d]=%g must be finite and > 0", d, w->threshold[d]);
        if (w->loop[d] > 1) return fail(c, IRLOSC_ERR_ARG, "waypoints: loop[%d]=%d must be 0 or 1", d, (int)w->loop[d]);
        for (int b = 0; b < w->nb; ++b)
            for (int i = 0; i < w->count[d] * 3; ++i) {
                const size_t e = (((size_t)b * nd + d) * wmax) * 3 + i;
                if (!std::isfinite(dense[e] = xyz[e]))
                    return fail(c, IRLOSC_ERR_ARG, "waypoints: waypoint %d of device %d, robot %d is not finite", i / 3, d, b);
            }
    }
    if (B > std::max(0, s.targets))
        return fail(c, IRLOSC_ERR_STATE, "slot %d holds targets for %d instances, waypoints given for %d: irlosc_set_targets first", slot,
                    std::max(0, s.targets), B);
    HIPCHK(c, hipSetDevice(c->cfg.hip_device));
    Program& p = s.prog;
    p.end();           // (none until the new ones are in their buffers; the paths write the targets from here on: an action list ends)
    s.episodes.end();  // (set on the program this call replaces)
    const std::vector<double> tab = walk_table(dense.data(), w->nb, E);
    const size_t bytes = tab.size() * sizeof(double), state = p.wp_words((size_t)nd * c->cfg.max_batch) * sizeof(int32_t);
    if (!got(p.wp_table.reserve(bytes)) || !got(p.wp_i.ensure(state)))
        return fail(c, IRLOSC_ERR_HIP, "out of device memory for the waypoint paths of slot %d (%zu bytes)", slot, bytes + state);
    const WaypointArgs init = waypoint_args(c, s, B, *w, nullptr, 0);
    rc = setter_upload(c, {{p.wp_table, tab.data(), bytes}}, c->cfg.dtype == IRLOSC_F64 ? launch_waypoints<double> : launch_waypoints<float>, &init);
    if (!rc) p.paths(B, *w);
    return rc;
}

extern "C" int irlosc_download_waypoint_state(irlosc_ctx* c, int32_t slot, int32_t B, int32_t* index, uint32_t* arrivals, int32_t* last_tick) {
    if (!c) return IRLOSC_ERR_ARG;
    int rc = check_slot(c, slot, B);
    if (!rc) rc = check_program(c, slot, B, Program::PATHS);
    if (rc) return rc;
    const Program& p = c->slot[slot].prog;
    if (B == 0) return IRLOSC_OK;
    HIPCHK(c, hipSetDevice(c->cfg.hip_device));
    const size_t nd = (size_t)c->cfg.ndev, plane = nd * c->cfg.max_batch;      // planes [ndev][max_batch] on the device -> [B][ndev] each for the caller
    return download_state(c, B, nullptr, 0, {}, p.wp_i, p.wp_words(plane), {{index, p.index(plane), nd, nd, 0, 1},
                          {(int32_t*)arrivals, p.arrivals(plane), nd, nd, 0, 1}, {last_tick, p.last_tick(plane), nd, nd, 0, 1}});
}

// ---- external pushes of the rollout (osc_push.hpp) ----------------------------------------------------------------------------
extern "C" int irlosc_set_pushes(irlosc_ctx* c, int32_t slot, int32_t B, const irlosc_pushes* d, const double* wrench) {
    if (!c) return IRLOSC_ERR_ARG;
    int rc = check_slot(c, slot, B);
    if (rc) return rc;
    Slot& s = c->slot[slot];
    if (!d) { s.push.end(); return IRLOSC_OK; }
    const int nd = c->cfg.ndev, P = d->n_pushes;
    if (P < 1 || P > IRLOSC_MAX_PUSHES) return fail(c, IRLOSC_ERR_ARG, "pushes: n_pushes=%d out of [1,%d]", P, IRLOSC_MAX_PUSHES);
    if (B < 1) return fail(c, IRLOSC_ERR_ARG, "pushes: B=%d must be >= 1", B);
    if (d->nb != 1 && d->nb != B) return fail(c, IRLOSC_ERR_ARG, "pushes: nb=%d must be 1 or B=%d", d->nb, B);
    for (int p = 0; p < P; ++p) {
        if (d->dev[p] < 0 || d->dev[p] >= nd) return fail(c, IRLOSC_ERR_ARG, "pushes: dev[%d]=%d out of [0,%d)", p, d->dev[p], nd);
        if (d->tick0[p] < 0 || d->tick0[p] >= d->tick1[p])
            return fail(c, IRLOSC_ERR_ARG, "pushes: window [%d,%d) of push %d must hold 0 <= tick0 < tick1", d->tick0[p], d->tick1[p], p);
        if (d->apply[p] > 1 || d->sense[p] > 1 || !(d->apply[p] | d->sense[p]))
            return fail(c, IRLOSC_ERR_ARG, "pushes: apply[%d]=%d, sense[%d]=%d must be 0 or 1 and not both 0", p, (int)d->apply[p], p, (int)d->sense[p]);
    }
    if (!wrench) return fail(c, IRLOSC_ERR_ARG, "pushes: wrench is NULL");
    const size_t E = (size_t)P * 6;
    for (size_t i = 0; i < (size_t)d->nb * E; ++i)
        if (!std::isfinite(wrench[i]))
            return fail(c, IRLOSC_ERR_ARG, "pushes: wrench of push %zu, robot %zu is not finite", i % E / 6, i / E);
    if (!c->model.in_force) return fail(c, IRLOSC_ERR_STATE, "irlosc_set_model has not been called");
    if (s.episodes.robots)
        return fail(c, IRLOSC_ERR_STATE, "slot %d has episodes: the pushes' windows are the slot's ticks, not a robot's (irlosc_set_episodes with NULL first)", slot);
    HIPCHK(c, hipSetDevice(c->cfg.hip_device));
    Pushes& ps = s.push;
    ps.end();          // (none until the new ones are in their table)
    const std::vector<double> tab = walk_table(wrench, d->nb, E);
    const size_t bytes = tab.size() * sizeof(double);
    if (!got(ps.table.reserve(bytes))) return fail(c, IRLOSC_ERR_HIP, "out of device memory for the pushes of slot %d (%zu bytes)", slot, bytes);
    rc = setter_upload(c, {{ps.table, tab.data(), bytes}});
    if (!rc) ps.set(B, *d);
    return rc;
}

// ---- compliant walls of the rollout (osc_wall.hpp) ------------------------------------------------------------------------------
extern "C" int irlosc_set_walls(irlosc_ctx* c, int32_t slot, int32_t B, const irlosc_walls* d, const double* table) {
    if (!c) return IRLOSC_ERR_ARG;
    int rc = check_slot(c, slot, B);
    if (rc) return rc;
    Slot& s = c->slot[slot];
    if (!d) { s.walls.end(); return IRLOSC_OK; }
    const int nd = c->cfg.ndev, W = d->n_walls;
    if (W < 1 || W > IRLOSC_MAX_WALLS) return fail(c, IRLOSC_ERR_ARG, "walls: n_walls=%d out of [1,%d]", W, IRLOSC_MAX_WALLS);
    if (B < 1) return fail(c, IRLOSC_ERR_ARG, "walls: B=%d must be >= 1", B);
    if (d->nb != 1 && d->nb != B) return fail(c, IRLOSC_ERR_ARG, "walls: nb=%d must be 1 or B=%d", d->nb, B);
    for (int w = 0; w < W; ++w)
        if (d->dev[w] < 0 || d->dev[w] >= nd) return fail(c, IRLOSC_ERR_ARG, "walls: dev[%d]=%d out of [0,%d)", w, d->dev[w], nd);
    if (!table) return fail(c, IRLOSC_ERR_ARG, "walls: table is NULL");
    const size_t E = (size_t)W * 8;
    for (size_t i = 0; i < (size_t)d->nb * E; ++i)
        if (!std::isfinite(table[i]))
            return fail(c, IRLOSC_ERR_ARG, "walls: word %zu of wall %zu, robot %zu is not finite", i % 8, i % E / 8, i / E);
    for (size_t i = 0; i < (size_t)d->nb * W; ++i) {
        const double* r = table + i * 8;
        const double n2 = r[0] * r[0] + r[1] * r[1] + r[2] * r[2];
        if (std::fabs(n2 - 1.0) > 1e-12)
            return fail(c, IRLOSC_ERR_ARG, "walls: the normal of wall %zu, robot %zu is no unit vector (|n|^2 - 1 = %g)", i % W, i / W, n2 - 1.0);
        if (r[4] < 0.0 || r[5] < 0.0 || r[6] < 0.0)
            return fail(c, IRLOSC_ERR_ARG, "walls: radius %g, stiffness %g, damping %g of wall %zu, robot %zu must be >= 0", r[4], r[5], r[6], i % W, i / W);
    }
    if (!c->model.in_force) return fail(c, IRLOSC_ERR_STATE, "irlosc_set_model has not been called");
    HIPCHK(c, hipSetDevice(c->cfg.hip_device));
    Walls& ws = s.walls;
    ws.end();          // (none until the new ones are in their table and their state is reset)
    const std::vector<double> tab = walk_table(table, d->nb, E);
    const size_t bytes = tab.size() * sizeof(double), plane = (size_t)nd * c->cfg.max_batch;
    const size_t d_bytes = ws.d_words(plane) * sizeof(double), i_bytes = ws.i_words(plane) * sizeof(int32_t);
    if (!got(ws.table.reserve(bytes)) || !got(ws.st_d.ensure(d_bytes)) || !got(ws.st_i.ensure(i_bytes)))
        return fail(c, IRLOSC_ERR_HIP, "out of device memory for the walls of slot %d (%zu bytes)", slot, bytes + d_bytes + i_bytes);
    rc = setter_upload(c, {{ws.table, tab.data(), bytes}, {ws.st_d, nullptr, d_bytes, 0},                // force, max_depth = 0
                       {ws.contact_ticks(plane), nullptr, plane * sizeof(int32_t), 0},                   // contact_ticks = 0
                       {ws.first_tick(plane), nullptr, plane * sizeof(int32_t), 0xff}});                 // first_tick = -1
    if (!rc) ws.set(B, *d);
    return rc;
}

extern "C" int irlosc_download_wall_state(irlosc_ctx* c, int32_t slot, int32_t B, double* force, double* max_depth, int32_t* contact_ticks,
                                          int32_t* first_tick) {
    if (!c) return IRLOSC_ERR_ARG;
    int rc = check_slot(c, slot, B);
    if (!rc) rc = check_covers(c, slot, B, c->slot[slot].walls.robots, "walls", "cover", "irlosc_set_walls");
    if (rc) return rc;
    const Walls& ws = c->slot[slot].walls;
    if (B == 0) return IRLOSC_OK;
    HIPCHK(c, hipSetDevice(c->cfg.hip_device));
    const size_t nd = (size_t)c->cfg.ndev, plane = nd * c->cfg.max_batch;      // planes [ndev][max_batch] on the device -> [B][ndev](,3) for the caller
    return download_state(c, B, ws.st_d, ws.d_words(plane), {{force, ws.force(plane, 0), nd, nd * 3, 0, 3}, {force, ws.force(plane, 1), nd, nd * 3, 1, 3},
                          {force, ws.force(plane, 2), nd, nd * 3, 2, 3}, {max_depth, ws.max_depth(plane), nd, nd, 0, 1}},
                          ws.st_i, ws.i_words(plane), {{contact_ticks, ws.contact_ticks(plane), nd, nd, 0, 1}, {first_tick, ws.first_tick(plane), nd, nd, 0, 1}});
}

// ---- joint rows of the rollout (osc_joint.hpp) ------------------------------------------------------------------------------------
extern "C" int irlosc_set_joints(irlosc_ctx* c, int32_t slot, int32_t B, const irlosc_joint_rows* d, const double* table) {
    if (!c) return IRLOSC_ERR_ARG;
    int rc = check_slot(c, slot, B);
    if (rc) return rc;
    Slot& s = c->slot[slot];
    if (!d) { s.joints.end(); return IRLOSC_OK; }
    const int n = c->cfg.n, nd = c->cfg.ndev, R = d->n_rows;
    if (R < 1 || R > IRLOSC_MAX_JOINT_ROWS) return fail(c, IRLOSC_ERR_ARG, "joints: n_rows=%d out of [1,%d]", R, IRLOSC_MAX_JOINT_ROWS);
    if (B < 1) return fail(c, IRLOSC_ERR_ARG, "joints: B=%d must be >= 1", B);
    if (d->per_robot != 0 && d->per_robot != 1) return fail(c, IRLOSC_ERR_ARG, "joints: per_robot=%d must be 0 or 1", d->per_robot);
    for (int r = 0; r < R; ++r) {
        const int k = d->kind[r];
        if (k != IRLOSC_JOINT_LIMIT && k != IRLOSC_JOINT_COUPLE && k != IRLOSC_JOINT_DRIVE)
            return fail(c, IRLOSC_ERR_ARG, "joints: kind[%d]=%d is unknown", r, k);
        if (d->joint_a[r] < 0 || d->joint_a[r] >= n) return fail(c, IRLOSC_ERR_ARG, "joints: joint_a[%d]=%d out of [0,%d)", r, d->joint_a[r], n);
        if (k == IRLOSC_JOINT_COUPLE) {
            if (d->joint_b[r] < 0 || d->joint_b[r] >= n) return fail(c, IRLOSC_ERR_ARG, "joints: joint_b[%d]=%d out of [0,%d)", r, d->joint_b[r], n);
            if (d->joint_b[r] == d->joint_a[r]) return fail(c, IRLOSC_ERR_ARG, "joints: row %d couples hinge %d with itself", r, d->joint_a[r]);
        }
        if (k == IRLOSC_JOINT_DRIVE) {
            if (d->source[r] != IRLOSC_JOINT_SRC_CONST && d->source[r] != IRLOSC_JOINT_SRC_ACTION)
                return fail(c, IRLOSC_ERR_ARG, "joints: source[%d]=%d is unknown", r, d->source[r]);
            if (d->source[r] == IRLOSC_JOINT_SRC_ACTION && (d->dev[r] < 0 || d->dev[r] >= nd))
                return fail(c, IRLOSC_ERR_ARG, "joints: dev[%d]=%d out of [0,%d)", r, d->dev[r], nd);
        }
    }
    if (!table) return fail(c, IRLOSC_ERR_ARG, "joints: table is NULL");
    const int nb = d->per_robot ? B : 1;
    const size_t E = (size_t)R * 8;
    for (size_t i = 0; i < (size_t)nb * E; ++i)
        if (!std::isfinite(table[i]))
            return fail(c, IRLOSC_ERR_ARG, "joints: word %zu of row %zu, robot %zu is not finite", i % 8, i % E / 8, i / E);
    for (size_t i = 0; i < (size_t)nb * R; ++i) {
        const double* t = table + i * 8;
        const int k = d->kind[i % R];
        if (k == IRLOSC_JOINT_LIMIT && !(t[0] < t[1]))
            return fail(c, IRLOSC_ERR_ARG, "joints: the range [%g, %g] of row %zu, robot %zu is empty (lo >= hi)", t[0], t[1], i % R, i / R);
        const double kk = k == IRLOSC_JOINT_LIMIT ? t[2] : t[4], cc = k == IRLOSC_JOINT_LIMIT ? t[3] : t[5];
        if (k != IRLOSC_JOINT_DRIVE && (kk < 0.0 || cc < 0.0))
            return fail(c, IRLOSC_ERR_ARG, "joints: stiffness %g, damping %g of row %zu, robot %zu must be >= 0", kk, cc, i % R, i / R);
    }
    if (!c->model.in_force) return fail(c, IRLOSC_ERR_STATE, "irlosc_set_model has not been called");
    HIPCHK(c, hipSetDevice(c->cfg.hip_device));
    Joints& js = s.joints;
    js.end();          // (none until the new ones are in their table and their state is reset)
    const std::vector<double> tab = walk_table(table, nb, E);
    const size_t bytes = tab.size() * sizeof(double), Bm = (size_t)c->cfg.max_batch;
    const size_t d_bytes = js.d_words(Bm, R) * sizeof(double), i_bytes = js.i_words(Bm, R) * sizeof(int32_t);
    if (!got(js.table.reserve(bytes)) || !got(js.st_d.reserve(d_bytes)) || !got(js.st_i.reserve(i_bytes)))
        return fail(c, IRLOSC_ERR_HIP, "out of device memory for the joint rows of slot %d (%zu bytes)", slot, bytes + d_bytes + i_bytes);
    rc = setter_upload(c, {{js.table, tab.data(), bytes}, {js.st_d, nullptr, d_bytes, 0}, {js.st_i, nullptr, i_bytes, 0}});      // every word of the state = 0
    if (!rc) js.set(B, *d);
    return rc;
}

extern "C" int irlosc_download_joint_state(irlosc_ctx* c, int32_t slot, int32_t B, double* tau, double* max_violation, int32_t* active_ticks,
                                           double* ctrl) {
    if (!c) return IRLOSC_ERR_ARG;
    int rc = check_slot(c, slot, B);
    if (!rc) rc = check_covers(c, slot, B, c->slot[slot].joints.robots, "joint rows", "cover", "irlosc_set_joints");
    if (rc) return rc;
    const Joints& js = c->slot[slot].joints;
    if (B == 0) return IRLOSC_OK;
    HIPCHK(c, hipSetDevice(c->cfg.hip_device));
    const size_t n = (size_t)c->cfg.n, R = (size_t)js.d.n_rows, Bm = (size_t)c->cfg.max_batch;      // rows [max_batch] on the device -> [B][n], [B][R] for the caller
    return download_state(c, B, js.st_d, js.d_words(Bm, R), {{tau, js.tau(Bm), n, n, 0, 1}, {max_violation, js.max_violation(Bm), R, R, 0, 1},
                          {ctrl, js.ctrl(Bm, R), R, R, 0, 1}}, js.st_i, js.i_words(Bm, R), {{active_ticks, js.active_ticks(Bm), R, R, 0, 1}});
}

// ---- action objects of the rollout (osc_object.hpp) ---------------------------------------------------------------------------------
extern "C" int irlosc_set_objects(irlosc_ctx* c, int32_t slot, int32_t B, const irlosc_objects* d, const double* pose0) {
    if (!c) return IRLOSC_ERR_ARG;
    int rc = check_slot(c, slot, B);
    if (rc) return rc;
    Slot& s = c->slot[slot];
    if (!d) { s.objects.end(); s.loads.end(); s.prog.aimless(); return IRLOSC_OK; }
    const int n = c->cfg.n, nd = c->cfg.ndev, NO = d->n_objects, NG = d->n_grippers, NM = d->n_mates, V = d->n_variants;
    if (NO < 1 || NO > IRLOSC_MAX_OBJECTS) return fail(c, IRLOSC_ERR_ARG, "objects: n_objects=%d out of [1,%d]", NO, IRLOSC_MAX_OBJECTS);
    if (NG < 1 || NG > IRLOSC_MAX_GRIPPERS) return fail(c, IRLOSC_ERR_ARG, "objects: n_grippers=%d out of [1,%d]", NG, IRLOSC_MAX_GRIPPERS);
    if (NM < 0 || NM > IRLOSC_MAX_MATES) return fail(c, IRLOSC_ERR_ARG, "objects: n_mates=%d out of [0,%d]", NM, IRLOSC_MAX_MATES);
    if (V < 1 || V > IRLOSC_MAX_EPISODE_STARTS) return fail(c, IRLOSC_ERR_ARG, "objects: n_variants=%d out of [1,%d]", V, IRLOSC_MAX_EPISODE_STARTS);
    if (B < 1) return fail(c, IRLOSC_ERR_ARG, "objects: B=%d must be >= 1", B);
    for (int g = 0; g < NG; ++g) {
        if (d->dev[g] < 0 || d->dev[g] >= nd) return fail(c, IRLOSC_ERR_ARG, "objects: dev[%d]=%d out of [0,%d)", g, d->dev[g], nd);
        if (d->joint[g] < 0 || d->joint[g] >= n) return fail(c, IRLOSC_ERR_ARG, "objects: joint[%d]=%d out of [0,%d)", g, d->joint[g], n);
        if (d->sign[g] != 1 && d->sign[g] != -1) return fail(c, IRLOSC_ERR_ARG, "objects: sign[%d]=%d must be +1 or -1", g, d->sign[g]);
        bool fin = std::isfinite(d->q_close[g]) && std::isfinite(d->q_open[g]);
        for (int i = 0; i < 3; ++i) fin = fin && std::isfinite(d->grip_xyz[g][i]);
        if (!fin) return fail(c, IRLOSC_ERR_ARG, "objects: q_close / q_open / grip_xyz of gripper %d must be finite", g);
        if (!(d->sign[g] * d->q_open[g] < d->sign[g] * d->q_close[g]))
            return fail(c, IRLOSC_ERR_ARG, "objects: gripper %d opens at %g and closes at %g: sign q_open must lie below sign q_close", g, d->q_open[g], d->q_close[g]);
    }
    for (int o = 0; o < NO; ++o)
        if (!(std::isfinite(d->radius[o]) && d->radius[o] >= 0.0)) return fail(c, IRLOSC_ERR_ARG, "objects: radius[%d]=%g must be finite and >= 0", o, d->radius[o]);
    for (int m = 0; m < NM; ++m) {
        if (d->plug[m] < 0 || d->plug[m] >= NO || d->socket[m] < 0 || d->socket[m] >= NO)
            return fail(c, IRLOSC_ERR_ARG, "objects: plug[%d]=%d, socket[%d]=%d out of [0,%d)", m, d->plug[m], m, d->socket[m], NO);
        if (d->plug[m] == d->socket[m]) return fail(c, IRLOSC_ERR_ARG, "objects: mate %d plugs object %d into itself", m, d->plug[m]);
        bool fin = true;
        for (int i = 0; i < 3; ++i) fin = fin && std::isfinite(d->seat_xyz[m][i]);
        for (int i = 0; i < 4; ++i) fin = fin && std::isfinite(d->seat_quat[m][i]);
        if (!fin) return fail(c, IRLOSC_ERR_ARG, "objects: seat_xyz / seat_quat of mate %d must be finite", m);
        if (!(std::isfinite(d->tol_xyz[m]) && d->tol_xyz[m] > 0.0)) return fail(c, IRLOSC_ERR_ARG, "objects: tol_xyz[%d]=%g must be finite and > 0", m, d->tol_xyz[m]);
        if (!(d->min_abs_dot[m] >= 0.0 && d->min_abs_dot[m] <= 1.0)) return fail(c, IRLOSC_ERR_ARG, "objects: min_abs_dot[%d]=%g out of [0,1]", m, d->min_abs_dot[m]);
    }
    if (!pose0) return fail(c, IRLOSC_ERR_ARG, "objects: pose0 is NULL");
    const size_t E = (size_t)NO * 7;
    for (size_t i = 0; i < (size_t)V * B * E; ++i)
        if (!std::isfinite(pose0[i]))
            return fail(c, IRLOSC_ERR_ARG, "objects: start pose of object %zu, robot %zu, variant %zu is not finite", i % E / 7, i / E % B, i / E / B);
    if (!c->model.in_force) return fail(c, IRLOSC_ERR_STATE, "irlosc_set_model has not been called");
    if (B > std::max(0, s.coords))
        return fail(c, IRLOSC_ERR_STATE, "slot %d holds joint coordinates of %d instances, objects given for %d: irlosc_upload_q first", slot, std::max(0, s.coords), B);
    HIPCHK(c, hipSetDevice(c->cfg.hip_device));
    Objects& os = s.objects;
    os.end();          // (none until the new ones are in their table and their state is reset; the refs named the old ones)
    s.loads.end();     // (... and the loads described them)
    s.prog.aimless();
    // the start poses, every variant in the walk's layout even for a lone robot: [V][walk wave][NO 7][64]
    const size_t vstride = ((size_t)B + 63) / 64 * E * 64;
    std::vector<double> tab((size_t)V * vstride, 0.0);
    for (size_t v = 0; v < (size_t)V; ++v)
        for (size_t b = 0; b < (size_t)B; ++b)
            for (size_t k = 0; k < E; ++k) tab[v * vstride + ((b / 64) * E + k) * 64 + b % 64] = pose0[(v * B + b) * E + k];
    const size_t bytes = tab.size() * sizeof(double), Bm = (size_t)c->cfg.max_batch;
    const size_t d_bytes = os.d_words(Bm) * sizeof(double), i_bytes = os.i_words(Bm) * sizeof(int32_t);
    if (!got(os.table.reserve(bytes)) || !got(os.st_d.ensure(d_bytes)) || !got(os.st_i.ensure(i_bytes)))
        return fail(c, IRLOSC_ERR_HIP, "out of device memory for the action objects of slot %d (%zu bytes)", slot, bytes + d_bytes + i_bytes);
    const ObjectArgs init = object_args(c, s, B, *d, nullptr);
    rc = setter_upload(c, {{os.table, tab.data(), bytes}, {os.st_d, nullptr, d_bytes, 0}, {os.st_i, nullptr, i_bytes, 0}}, launch_objects, &init);
    if (!rc) os.set(B, *d, vstride);
    return rc;
}

extern "C" int irlosc_download_object_state(irlosc_ctx* c, int32_t slot, int32_t B, double* pose, int32_t* holder, double* rel,
                                            int32_t* grasp_tick, int32_t* release_tick, int32_t* mated_tick) {
    if (!c) return IRLOSC_ERR_ARG;
    int rc = check_slot(c, slot, B);
    if (!rc) rc = check_covers(c, slot, B, c->slot[slot].objects.robots, "action objects", "cover", "irlosc_set_objects");
    if (rc) return rc;
    const Objects& os = c->slot[slot].objects;
    if (B == 0) return IRLOSC_OK;
    HIPCHK(c, hipSetDevice(c->cfg.hip_device));
    const size_t NO = (size_t)os.d.n_objects, NM = (size_t)os.d.n_mates, Bm = (size_t)c->cfg.max_batch;      // rows [max_batch] -> [B][NO][7], [B][NO], [B][NM]
    return download_state(c, B, os.st_d, os.d_words(Bm), {{pose, os.pose(Bm), NO * 7, NO * 7, 0, 1}, {rel, os.rel(Bm), NO * 7, NO * 7, 0, 1}},
                          os.st_i, os.i_words(Bm), {{holder, os.holder(Bm), NO, NO, 0, 1}, {grasp_tick, os.grasp_tick(Bm), NO, NO, 0, 1},
                          {release_tick, os.release_tick(Bm), NO, NO, 0, 1}, {mated_tick, os.mated_tick(Bm), NM, NM, 0, 1}});
}

// ---- the carried objects' weight (osc_object_load.hpp) ---------------------------------------------------------------------------------
extern "C" int irlosc_set_object_loads(irlosc_ctx* c, int32_t slot, int32_t B, const irlosc_object_loads* d, const double* table) {
    if (!c) return IRLOSC_ERR_ARG;
    int rc = check_slot(c, slot, B);
    if (rc) return rc;
    Slot& s = c->slot[slot];
    if (!d) { s.loads.end(); return IRLOSC_OK; }      // (the objects and their state are not touched)
    if (B < 1) return fail(c, IRLOSC_ERR_ARG, "object loads: B=%d must be >= 1", B);
    if (d->per_robot != 0 && d->per_robot != 1) return fail(c, IRLOSC_ERR_ARG, "object loads: per_robot=%d must be 0 or 1", d->per_robot);
    if (d->reserved != 0) return fail(c, IRLOSC_ERR_ARG, "object loads: reserved must be 0");
    for (int i = 0; i < 3; ++i)
        if (!std::isfinite(d->gravity[i])) return fail(c, IRLOSC_ERR_ARG, "object loads: gravity[%d] is not finite", i);
    if (!table) return fail(c, IRLOSC_ERR_ARG, "object loads: table is NULL");
    const int NO = s.objects.count();      // (the table's width is the objects': without them there is nothing to read it by)
    if (!NO) return fail(c, IRLOSC_ERR_STATE, "slot %d has no action objects (irlosc_set_objects)", slot);
    const int nb = d->per_robot ? B : 1;
    const size_t E = (size_t)NO * 4;
    for (size_t i = 0; i < (size_t)nb * E; ++i) {
        if (!std::isfinite(table[i]))
            return fail(c, IRLOSC_ERR_ARG, "object loads: word %zu of object %zu, robot %zu is not finite", i % 4, i % E / 4, i / E);
        if (i % 4 == 0 && table[i] < 0.0)
            return fail(c, IRLOSC_ERR_ARG, "object loads: mass %g of object %zu, robot %zu must be >= 0", table[i], i % E / 4, i / E);
    }
    if (B > s.objects.robots)
        return fail(c, IRLOSC_ERR_STATE, "slot %d: its action objects cover %d robots, loads given for %d", slot, s.objects.robots, B);
    HIPCHK(c, hipSetDevice(c->cfg.hip_device));
    Loads& ls = s.loads;
    ls.end();          // (none until the new ones are in their table and their state is reset)
    const std::vector<double> tab = walk_table(table, nb, E);
    const size_t bytes = tab.size() * sizeof(double), Bm = (size_t)c->cfg.max_batch;
    const size_t d_bytes = ls.d_words(Bm) * sizeof(double), i_bytes = ls.i_words(Bm) * sizeof(int32_t);
    if (!got(ls.table.reserve(bytes)) || !got(ls.st_d.ensure(d_bytes)) || !got(ls.st_i.ensure(i_bytes)))
        return fail(c, IRLOSC_ERR_HIP, "out of device memory for the object loads of slot %d (%zu bytes)", slot, bytes + d_bytes + i_bytes);
    rc = setter_upload(c, {{ls.table, tab.data(), bytes}, {ls.st_d, nullptr, d_bytes, 0}, {ls.st_i, nullptr, i_bytes, 0}});      // load, carry_ticks = 0
    irlosc_object_loads in_force = *d;
    in_force.per_robot = nb > 1;      // (walk_table lays a lone robot's table out as the shared one)
    if (!rc) ls.set(B, in_force);
    return rc;
}

extern "C" int irlosc_download_object_load_state(irlosc_ctx* c, int32_t slot, int32_t B, double* load, int32_t* carry_ticks) {
    if (!c) return IRLOSC_ERR_ARG;
    int rc = check_slot(c, slot, B);
    if (!rc) rc = check_covers(c, slot, B, c->slot[slot].loads.robots, "object loads", "cover", "irlosc_set_object_loads");
    if (rc) return rc;
    const Loads& ls = c->slot[slot].loads;
    if (B == 0) return IRLOSC_OK;
    HIPCHK(c, hipSetDevice(c->cfg.hip_device));
    const size_t NG = (size_t)c->slot[slot].objects.d.n_grippers, Bm = (size_t)c->cfg.max_batch;      // rows [max_batch] -> [B][NG][6], [B][NG]
    return download_state(c, B, ls.st_d, ls.d_words(Bm), {{load, ls.load(Bm), NG * 6, NG * 6, 0, 1}}, ls.st_i, ls.i_words(Bm),
                          {{carry_ticks, ls.carry_ticks(Bm), NG, NG, 0, 1}});
}

extern "C" int irlosc_set_action_refs(irlosc_ctx* c, int32_t slot, const irlosc_action_refs* r) {
    if (!c) return IRLOSC_ERR_ARG;
    int rc = check_slot(c, slot, 0);
    if (rc) return rc;
    Slot& s = c->slot[slot];
    if (!r) { s.prog.aimless(); return IRLOSC_OK; }
    const int NO = s.objects.count();
    for (int i = 0; s.prog.kind == Program::LIST && NO && i < s.prog.al.n_actions; ++i) {
        if (s.prog.al.kind[i] != IRLOSC_ACTION_WP) continue;
        if (r->xyz_obj[i] < -1 || r->xyz_obj[i] >= NO || r->quat_obj[i] < -1 || r->quat_obj[i] >= NO)
            return fail(c, IRLOSC_ERR_ARG, "action refs: xyz_obj[%d]=%d, quat_obj[%d]=%d must be -1 or an object in [0,%d)", i, r->xyz_obj[i], i, r->quat_obj[i], NO);
    }
    if (s.prog.kind != Program::LIST) return fail(c, IRLOSC_ERR_STATE, "slot %d has no action list (irlosc_set_action_list)", slot);
    if (!NO) return fail(c, IRLOSC_ERR_STATE, "slot %d has no action objects (irlosc_set_objects)", slot);
    if (s.objects.robots < s.prog.robots)
        return fail(c, IRLOSC_ERR_STATE, "slot %d: its action objects cover %d robots, its action list %d", slot, s.objects.robots, s.prog.robots);
    irlosc_action_refs clean;
    for (int i = 0; i < IRLOSC_MAX_ACTIONS; ++i) {
        const bool wp = i < s.prog.al.n_actions && s.prog.al.kind[i] == IRLOSC_ACTION_WP;
        clean.xyz_obj[i] = wp ? r->xyz_obj[i] : -1; clean.quat_obj[i] = wp ? r->quat_obj[i] : -1;
    }
    s.prog.aims(clean);
    return IRLOSC_OK;
}

// ---- the WP / GRIP action list of the rollout (osc_action.hpp) ---------------------------------------------------------------
extern "C" int irlosc_set_action_list(irlosc_ctx* c, int32_t slot, int32_t B, const irlosc_action_list* d, const double* pose) {
    if (!c) return IRLOSC_ERR_ARG;
    int rc = check_slot(c, slot, B);
    if (rc) return rc;
    Slot& s = c->slot[slot];
    if (!d) { if (s.prog.kind == Program::LIST) s.episodes.end(); s.prog.end(Program::LIST); return IRLOSC_OK; }
    const int nd = c->cfg.ndev, A = d->n_actions;
    if (A < 1 || A > IRLOSC_MAX_ACTIONS) return fail(c, IRLOSC_ERR_ARG, "action list: n_actions=%d out of [1,%d]", A, IRLOSC_MAX_ACTIONS);
    if (B < 1) return fail(c, IRLOSC_ERR_ARG, "action list: B=%d must be >= 1", B);
    if (d->nb != 1 && d->nb != B) return fail(c, IRLOSC_ERR_ARG, "action list: nb=%d must be 1 or B=%d", d->nb, B);
    if (d->active_dev < 0 || d->active_dev >= nd) return fail(c, IRLOSC_ERR_ARG, "action list: active_dev=%d out of [0,%d)", d->active_dev, nd);
    if (d->passive_dev < -1 || d->passive_dev >= nd || d->passive_dev == d->active_dev)
        return fail(c, IRLOSC_ERR_ARG, "action list: passive_dev=%d must be -1 or a device in [0,%d) other than active_dev", d->passive_dev, nd);
    if (d->passive_hold_orientation != 0 && d->passive_hold_orientation != 1)
        return fail(c, IRLOSC_ERR_ARG, "action list: passive_hold_orientation=%d must be 0 or 1", d->passive_hold_orientation);
    for (int i = 0; i < 4; ++i)
        if (!std::isfinite(d->passive_quat[i])) return fail(c, IRLOSC_ERR_ARG, "action list: passive_quat[%d] is not finite", i);
    if (!pose) return fail(c, IRLOSC_ERR_ARG, "action list: pose is NULL");
    bool has_wp = false;
    for (int i = 0; i < A; ++i) {
        if (d->kind[i] != IRLOSC_ACTION_WP && d->kind[i] != IRLOSC_ACTION_GRIP)
            return fail(c, IRLOSC_ERR_ARG, "action list: kind[%d]=%d is neither WP nor GRIP", i, d->kind[i]);
        if (!std::isfinite(d->gripper_force[i])) return fail(c, IRLOSC_ERR_ARG, "action list: gripper_force[%d] is not finite", i);
        if (d->kind[i] == IRLOSC_ACTION_GRIP) {
            if (d->grip_ticks[i] < 1) return fail(c, IRLOSC_ERR_ARG, "action list: grip_ticks[%d]=%d must be >= 1", i, d->grip_ticks[i]);
            continue;
        }
        has_wp = true;
        if (d->xyz_from_start[i] != 0 && d->xyz_from_start[i] != 1)
            return fail(c, IRLOSC_ERR_ARG, "action list: xyz_from_start[%d]=%d must be 0 or 1", i, d->xyz_from_start[i]);
        if (!std::isfinite(d->kp[i]) || !std::isfinite(d->max_error[i]) || !std::isfinite(d->min_speed[i]) || !std::isfinite(d->max_speed[i]))
            return fail(c, IRLOSC_ERR_ARG, "action list: kp / max_error / min_speed / max_speed of action %d must be finite", i);
        if (d->min_speed[i] > d->max_speed[i])
            return fail(c, IRLOSC_ERR_ARG, "action list: min_speed[%d]=%g exceeds max_speed=%g", i, d->min_speed[i], d->max_speed[i]);
        for (int b = 0; b < d->nb; ++b)
            for (int w = 0; w < 7; ++w)
                if (!std::isfinite(pose[((size_t)b * A + i) * 7 + w]))
                    return fail(c, IRLOSC_ERR_ARG, "action list: pose of action %d, robot %d is not finite", i, b);
    }
    if (!c->model.in_force) return fail(c, IRLOSC_ERR_STATE, "irlosc_set_model has not been called");
    if (c->gains_nb == 0) return fail(c, IRLOSC_ERR_STATE, "irlosc_set_gains has not been called");
    if (B > std::max(0, s.targets))
        return fail(c, IRLOSC_ERR_STATE, "slot %d holds targets for %d instances, action list given for %d: irlosc_set_targets first", slot,
                    std::max(0, s.targets), B);
    HIPCHK(c, hipSetDevice(c->cfg.hip_device));
    // the gains in force, as stored: checked for the velocity limit the list sets, then broadcast or copied into the slot's own
    const size_t e = c->esz, rec = (size_t)nd * IRLOSC_GAIN_WORDS * e, nbg = (size_t)c->gains_nb;
    std::vector<unsigned char> g(nbg * rec), nk(nbg * e);
    HIPCHK(c, hipMemcpyAsync(g.data(), c->dgains, g.size(), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(nk.data(), c->dnullkv, nk.size(), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    auto word = [&](size_t b, int dev, int w) {
        const unsigned char* p = g.data() + b * rec + ((size_t)dev * IRLOSC_GAIN_WORDS + w) * e;
        double v; float f;
        if (e == 8) memcpy(&v, p, 8); else { memcpy(&f, p, 4); v = f; }
        return v;
    };
    for (size_t b = 0; has_wp && b < std::min(nbg, (size_t)B); ++b)
        if (word(b, d->active_dev, 11) == 0.0)
            return fail(c, IRLOSC_ERR_STATE, "action list: the gains in force have has_max_vel == 0 for device %d (robot %zu): the velocity limit "
                        "a WP sets would be ignored", d->active_dev, b);
    Program& p = s.prog;
    p.end(Program::LIST);      // (none until the new one is in its buffers; paths end when it is in force)
    s.episodes.end();          // (set on the program this call replaces)
    std::vector<unsigned char> gs((size_t)B * rec), nks((size_t)B * e);
    for (size_t b = 0; b < (size_t)B; ++b) {
        memcpy(gs.data() + b * rec, g.data() + (nbg > 1 ? b : 0) * rec, rec);
        memcpy(nks.data() + b * e, nk.data() + (nbg > 1 ? b : 0) * e, e);
    }
    const std::vector<double> tab = walk_table(pose, d->nb, (size_t)A * 7);
    const size_t bytes = tab.size() * sizeof(double), Bm = (size_t)c->cfg.max_batch;
    if (!got(p.al_table.reserve(bytes)) || !got(p.al_i.ensure(p.al_i_words(Bm) * sizeof(int32_t))) || !got(p.al_d.ensure(p.al_d_words(Bm) * sizeof(double))) ||
        !got(p.al_gains.ensure(Bm * rec)) || !got(p.al_nullkv.ensure(Bm * e)))
        return fail(c, IRLOSC_ERR_HIP, "out of device memory for the action list of slot %d", slot);
    const ActionArgs init = action_args(c, s, B, *d, nullptr, 0);
    rc = setter_upload(c, {{p.al_table, tab.data(), bytes}, {p.al_gains, gs.data(), gs.size()}, {p.al_nullkv, nks.data(), nks.size()}},
                       c->cfg.dtype == IRLOSC_F64 ? launch_actions<double> : launch_actions<float>, &init);
    if (!rc) p.list(B, *d);
    return rc;
}

extern "C" int irlosc_download_action_state(irlosc_ctx* c, int32_t slot, int32_t B, int32_t* action, int32_t* grip_left, double* err,
                                            double* max_vel0, double* gripper_force, int32_t* finished_tick) {
    if (!c) return IRLOSC_ERR_ARG;
    int rc = check_slot(c, slot, B);
    if (!rc) rc = check_program(c, slot, B, Program::LIST);
    if (rc) return rc;
    const Program& p = c->slot[slot].prog;
    if (B == 0) return IRLOSC_OK;
    HIPCHK(c, hipSetDevice(c->cfg.hip_device));
    const size_t Bm = (size_t)c->cfg.max_batch;
    int32_t* di[3] = {action, grip_left, finished_tick};  const int32_t* si[3] = {p.action(Bm), p.grip_left(Bm), p.finished_tick(Bm)};
    for (int i = 0; i < 3; ++i)
        if (di[i]) HIPCHK(c, hipMemcpyAsync(di[i], si[i], (size_t)B * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    double* dd[3] = {err, max_vel0, gripper_force};  const double* sd[3] = {p.err(Bm), p.max_vel0(Bm), p.gripper_force(Bm)};
    for (int i = 0; i < 3; ++i)
        if (dd[i]) HIPCHK(c, hipMemcpyAsync(dd[i], sd[i], (size_t)B * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return IRLOSC_OK;
}

// ---- the motion of the list in force: INTERP moves and seeded target noise (osc_action.hpp: MOTION; osc_rng.hpp) -----------------------
extern "C" int irlosc_set_action_motion(irlosc_ctx* c, int32_t slot, const irlosc_action_motion* m, const uint32_t* draw0) {
    if (!c) return IRLOSC_ERR_ARG;
    int rc = check_slot(c, slot, 0);
    if (rc) return rc;
    Slot& s = c->slot[slot];
    Program& p = s.prog;
    if (!m) { p.still(); return IRLOSC_OK; }
    for (int i = 0; p.kind == Program::LIST && i < p.al.n_actions; ++i) {
        const int32_t st = m->steps[i];
        const double mean = m->noise_mean[i], sd = m->noise_std[i];
        if (p.al.kind[i] != IRLOSC_ACTION_WP) {
            if (st != 0 || mean != 0.0 || sd != 0.0)      // (a NaN is not 0)
                return fail(c, IRLOSC_ERR_ARG, "action motion: action %d is a GRIP: steps=%d, noise_mean=%g, noise_std=%g must be 0", i, st, mean, sd);
            continue;
        }
        if (st < 0 || st > (1 << 20)) return fail(c, IRLOSC_ERR_ARG, "action motion: steps[%d]=%d out of [0,%d]", i, st, 1 << 20);
        if (!std::isfinite(mean)) return fail(c, IRLOSC_ERR_ARG, "action motion: noise_mean[%d] is not finite", i);
        if (!std::isfinite(sd) || sd < 0.0) return fail(c, IRLOSC_ERR_ARG, "action motion: noise_std[%d]=%g must be finite and >= 0", i, sd);
    }
    if (p.kind != Program::LIST) return fail(c, IRLOSC_ERR_STATE, "slot %d has no action list (irlosc_set_action_list)", slot);
    HIPCHK(c, hipSetDevice(c->cfg.hip_device));
    const size_t Bm = (size_t)c->cfg.max_batch, B = (size_t)p.robots;
    irlosc_action_motion clean;
    memset(&clean, 0, sizeof clean);
    for (int i = 0; i < p.al.n_actions; ++i) { clean.steps[i] = m->steps[i]; clean.noise_mean[i] = m->noise_mean[i]; clean.noise_std[i] = m->noise_std[i]; }
    clean.seed = m->seed;
    p.still();                 // (none until the new one's state is in its buffers)
    if (!got(p.am_i.ensure(p.am_i_words(Bm) * sizeof(int32_t))) || !got(p.am_d.ensure(p.am_d_words(Bm) * sizeof(double))))
        return fail(c, IRLOSC_ERR_HIP, "out of device memory for the action motion of slot %d", slot);
    rc = setter_upload(c, {{p.am_i.get(), nullptr, p.am_i_words(Bm) * sizeof(int32_t), 0}, {p.am_d.get(), nullptr, p.am_d_words(Bm) * sizeof(double), 0},
                           {p.m_draws(Bm), draw0, draw0 ? B * sizeof(uint32_t) : 0, 0}});
    if (!rc) p.moves(clean);
    return rc;
}

extern "C" int irlosc_download_action_motion_state(irlosc_ctx* c, int32_t slot, int32_t B, int32_t* step, uint32_t* draws, double* origin, double* goal) {
    if (!c) return IRLOSC_ERR_ARG;
    int rc = check_slot(c, slot, B);
    if (!rc) rc = check_program(c, slot, B, Program::LIST);
    if (rc) return rc;
    const Program& p = c->slot[slot].prog;
    if (!p.motion) return fail(c, IRLOSC_ERR_STATE, "slot %d: its action list has no motion (irlosc_set_action_motion)", slot);
    if (B == 0) return IRLOSC_OK;
    HIPCHK(c, hipSetDevice(c->cfg.hip_device));
    const size_t Bm = (size_t)c->cfg.max_batch;      // rows [max_batch] -> [B], [B], [B][7], [B][7]
    return download_state(c, B, p.am_d, p.am_d_words(Bm), {{origin, p.m_origin(Bm), 7, 7, 0, 1}, {goal, p.m_goal(Bm), 7, 7, 0, 1}},
                          p.am_i, p.am_i_words(Bm), {{step, p.m_step(Bm), 1, 1, 0, 1}, {(int32_t*)draws, (const int32_t*)p.m_draws(Bm), 1, 1, 0, 1}});
}

// The rig of a stream or of a policy (the same fields, the same rules): IRLOSC_ERR_ARG with `what` in front of the reason
template <class D>
static int check_rig(irlosc_ctx* c, const char* what, int nd, const D* d) {
    if (!std::isfinite(d->increment)) return fail(c, IRLOSC_ERR_ARG, "%s: increment is not finite", what);
    bool any = false;
    for (int k = 0; k < IRLOSC_MAX_DEV; ++k) {
        const int kind = d->kind[k];
        if (kind != IRLOSC_TELEOP_NONE && kind != IRLOSC_TELEOP_RIGID && kind != IRLOSC_TELEOP_HEADING)
            return fail(c, IRLOSC_ERR_ARG, "%s: kind[%d]=%d is none of NONE, RIGID, HEADING", what, k, kind);
        if (kind != IRLOSC_TELEOP_NONE && k >= nd) return fail(c, IRLOSC_ERR_ARG, "%s: kind[%d]=%d on a device >= ndev=%d", what, k, kind, nd);
        any = any || kind != IRLOSC_TELEOP_NONE;
        if (kind == IRLOSC_TELEOP_RIGID) {
            double n2 = 0.0;
            for (int i = 0; i < 3; ++i)
                if (!std::isfinite(d->off_xyz[k][i])) return fail(c, IRLOSC_ERR_ARG, "%s: off_xyz[%d][%d] is not finite", what, k, i);
            for (int i = 0; i < 4; ++i) n2 += d->off_quat[k][i] * d->off_quat[k][i];
            if (!(std::fabs(n2 - 1.0) <= 1e-12))      // (a NaN or an infinity fails here too)
                return fail(c, IRLOSC_ERR_ARG, "%s: off_quat[%d] is not of unit length (|q|^2 = %.17g)", what, k, n2);
        }
        if (kind == IRLOSC_TELEOP_HEADING && !std::isfinite(d->heading_offset[k]))
            return fail(c, IRLOSC_ERR_ARG, "%s: heading_offset[%d] is not finite", what, k);
    }
    if (!any) return fail(c, IRLOSC_ERR_ARG, "%s: every device has kind NONE", what);
    return IRLOSC_OK;
}

// ---- the teleoperation stream of the rollout (osc_teleop.hpp) -------------------------------------------------------------------
extern "C" int irlosc_set_teleop_stream(irlosc_ctx* c, int32_t slot, int32_t B, const irlosc_teleop_stream* d, const double* readings,
                                        const double* origin) {
    if (!c) return IRLOSC_ERR_ARG;
    int rc = check_slot(c, slot, B);
    if (rc) return rc;
    Slot& s = c->slot[slot];
    if (!d) { s.prog.end(Program::STREAM); return IRLOSC_OK; }
    const int nd = c->cfg.ndev, T = d->ticks;
    if (T < 1 || T > IRLOSC_MAX_STREAM_TICKS) return fail(c, IRLOSC_ERR_ARG, "teleop stream: ticks=%d out of [1,%d]", T, IRLOSC_MAX_STREAM_TICKS);
    if (B < 1) return fail(c, IRLOSC_ERR_ARG, "teleop stream: B=%d must be >= 1", B);
    if (d->nb != 1 && d->nb != B) return fail(c, IRLOSC_ERR_ARG, "teleop stream: nb=%d must be 1 or B=%d", d->nb, B);
    if (d->nb_origin != 1 && d->nb_origin != B) return fail(c, IRLOSC_ERR_ARG, "teleop stream: nb_origin=%d must be 1 or B=%d", d->nb_origin, B);
    if (d->loop != 0 && d->loop != 1) return fail(c, IRLOSC_ERR_ARG, "teleop stream: loop=%d must be 0 or 1", d->loop);
    if ((rc = check_rig(c, "teleop stream", nd, d))) return rc;
    if (!readings || !origin) return fail(c, IRLOSC_ERR_ARG, "teleop stream: %s is NULL", !readings ? "readings" : "origin");
    const size_t E = (size_t)T * 6;
    for (size_t i = 0; i < (size_t)d->nb * E; ++i)
        if (!std::isfinite(readings[i])) return fail(c, IRLOSC_ERR_ARG, "teleop stream: reading %zu of robot %zu is not finite", i % E / 6, i / E);
    for (size_t i = 0; i < (size_t)d->nb_origin * 6; ++i)
        if (!std::isfinite(origin[i])) return fail(c, IRLOSC_ERR_ARG, "teleop stream: origin of robot %zu is not finite", i / 6);
    if (!c->model.in_force) return fail(c, IRLOSC_ERR_STATE, "irlosc_set_model has not been called");
    if (B > std::max(0, s.targets))
        return fail(c, IRLOSC_ERR_STATE, "slot %d holds targets for %d instances, teleop stream given for %d: irlosc_set_targets first", slot,
                    std::max(0, s.targets), B);
    if (s.episodes.robots)
        return fail(c, IRLOSC_ERR_STATE, "slot %d has episodes: a stream's reading index is the slot's tick, not a robot's (irlosc_set_episodes with NULL first)", slot);
    HIPCHK(c, hipSetDevice(c->cfg.hip_device));
    Program& p = s.prog;
    p.end();           // (none until the new one is in its buffers; the stream writes the targets from here on: paths or a list end)
    // what the init launch and the ticks read on the device: per-robot readings and origins; shared ones stay on the host
    std::vector<double> tab, org, shared;
    if (d->nb > 1) tab = walk_table(readings, d->nb, E); else shared.assign(readings, readings + E);
    if (d->nb_origin > 1) org = walk_table(origin, d->nb_origin, 6);
    const size_t Bm = (size_t)c->cfg.max_batch;
    if (!got(p.ts_pose.ensure(p.ts_words(Bm) * sizeof(double))) || !got(p.ts_table.reserve(tab.size() * sizeof(double))) ||
        !got(p.ts_origin.reserve(org.size() * sizeof(double))))
        return fail(c, IRLOSC_ERR_HIP, "out of device memory for the teleop stream of slot %d (%zu bytes)", slot,
                    (p.ts_words(Bm) + tab.size() + org.size()) * sizeof(double));
    const TeleopArgs init = teleop_args(c, s, B, *d, origin, -1);
    const auto launch = c->cfg.dtype == IRLOSC_F64 ? launch_teleop<double> : launch_teleop<float>;
    rc = setter_upload(c, {{p.ts_table, tab.data(), tab.size() * sizeof(double)}, {p.ts_origin, org.data(), org.size() * sizeof(double)}}, launch, &init);
    if (!rc) p.stream(B, *d, std::move(shared));
    return rc;
}

extern "C" int irlosc_download_teleop_state(irlosc_ctx* c, int32_t slot, int32_t B, double* pose, int32_t* tick) {
    if (!c) return IRLOSC_ERR_ARG;
    int rc = check_slot(c, slot, B);
    if (!rc) rc = check_program(c, slot, B, Program::STREAM);
    if (rc) return rc;
    const Program& p = c->slot[slot].prog;
    if (tick) *tick = p.tick;
    if (B == 0 || !pose) return IRLOSC_OK;
    HIPCHK(c, hipSetDevice(c->cfg.hip_device));
    const size_t Bm = (size_t)c->cfg.max_batch;      // rows [max_batch] on the device -> [B][6] for the caller
    return download_state(c, B, p.ts_pose, p.ts_words(Bm), {{pose, p.pose(Bm), 6, 6, 0, 1}}, nullptr, 0, {});
}

// ---- the policy of the rollout (osc_policy.hpp) -----------------------------------------------------------------------------------------
// The network of description d over n_in inputs as the kernel walks it, and (with `weights`) the packed copy `out`: per layer the
// fragments [output tile][k-step][64] -- lane l: W[16 ot + (l & 15)][4 ks + (l >> 4)], zero beyond the matrix -- then the bias padded to 16 ot
static PolicyNet policy_net(const irlosc_policy& d, int n_in, const float* weights = nullptr, std::vector<float>* out = nullptr) {
    PolicyNet net;
    memset(&net, 0, sizeof net);
    net.L = d.n_layers; net.n_in = n_in; net.n_out = d.n_out;
    size_t off = 0, src = 0;
    int in = n_in;
    for (int l = 0; l < d.n_layers; ++l) {
        const int o = l + 1 < d.n_layers ? d.width[l] : d.n_out, ks = (in + 3) / 4, ot = (o + 15) / 16;
        net.ksteps[l] = ks; net.otiles[l] = ot;
        net.woff[l] = (int32_t)off; net.boff[l] = (int32_t)(off + (size_t)ot * ks * 64);
        net.rows[l & 1] = std::max(net.rows[l & 1], 4 * ks);
        net.rows[(l & 1) ^ 1] = std::max(net.rows[(l & 1) ^ 1], 16 * ot);
        if (out) {
            out->resize(net.boff[l] + (size_t)ot * 16, 0.0f);
            for (int t = 0; t < ot; ++t)
                for (int k = 0; k < ks; ++k)
                    for (int ln = 0; ln < 64; ++ln) {
                        const int j = 16 * t + (ln & 15), i = 4 * k + (ln >> 4);
                        if (j < o && i < in) (*out)[off + ((size_t)t * ks + k) * 64 + ln] = weights[src + (size_t)j * in + i];
                    }
            for (int j = 0; j < o; ++j) (*out)[net.boff[l] + j] = weights[src + (size_t)o * in + j];
        }
        off = net.boff[l] + (size_t)ot * 16;
        src += (size_t)o * in + o;
        in = o;
    }
    return net;
}

extern "C" int irlosc_set_policy(irlosc_ctx* c, int32_t slot, int32_t B, const irlosc_policy* d, const float* weights, const double* origin) {
    if (!c) return IRLOSC_ERR_ARG;
    int rc = check_slot(c, slot, B);
    if (rc) return rc;
    Slot& s = c->slot[slot];
    if (!d) { if (s.prog.kind == Program::POLICY) s.episodes.end(); s.prog.end(Program::POLICY); return IRLOSC_OK; }
    const int nd = c->cfg.ndev, n = c->cfg.n, L = d->n_layers;
    constexpr uint32_t ALL = IRLOSC_OBS_QPOS | IRLOSC_OBS_QVEL | IRLOSC_OBS_EE_POSE | IRLOSC_OBS_TARGETS | IRLOSC_OBS_WRENCH | IRLOSC_OBS_PLATE | IRLOSC_OBS_OBJECT_POSE;
    if (B < 1) return fail(c, IRLOSC_ERR_ARG, "policy: B=%d must be >= 1", B);
    if (d->obs == 0 || (d->obs & ~ALL)) return fail(c, IRLOSC_ERR_ARG, "policy: obs=0x%x must name at least one of the IRLOSC_OBS_* channels and no other bit", d->obs);
    if (L < 1 || L > IRLOSC_POLICY_MAX_LAYERS) return fail(c, IRLOSC_ERR_ARG, "policy: n_layers=%d out of [1,%d]", L, IRLOSC_POLICY_MAX_LAYERS);
    for (int l = 0; l < IRLOSC_POLICY_MAX_LAYERS; ++l) {
        if (l < L - 1 && (d->width[l] < 1 || d->width[l] > IRLOSC_POLICY_MAX_WIDTH))
            return fail(c, IRLOSC_ERR_ARG, "policy: width[%d]=%d out of [1,%d]", l, d->width[l], IRLOSC_POLICY_MAX_WIDTH);
        if (l >= L - 1 && d->width[l] != 0) return fail(c, IRLOSC_ERR_ARG, "policy: width[%d]=%d behind the %d hidden layers must be 0", l, d->width[l], L - 1);
    }
    if (d->n_out != 6 && d->n_out != 7) return fail(c, IRLOSC_ERR_ARG, "policy: n_out=%d must be 6 or 7", d->n_out);
    if ((d->keep_obs != 0 && d->keep_obs != 1) || d->reserved != 0) return fail(c, IRLOSC_ERR_ARG, "policy: keep_obs=%d must be 0 or 1, reserved=%d must be 0", d->keep_obs, d->reserved);
    if (!(d->clip >= 0.0f) || !std::isfinite(d->clip)) return fail(c, IRLOSC_ERR_ARG, "policy: clip=%g must be finite and >= 0", (double)d->clip);
    if (d->nb_origin != 1 && d->nb_origin != B) return fail(c, IRLOSC_ERR_ARG, "policy: nb_origin=%d must be 1 or B=%d", d->nb_origin, B);
    if (d->n_out == 7) {
        if (d->grip_dev < 0 || d->grip_dev >= nd) return fail(c, IRLOSC_ERR_ARG, "policy: grip_dev=%d out of [0,%d)", d->grip_dev, nd);
        if (!std::isfinite(d->grip_close) || !std::isfinite(d->grip_open) || d->grip_close == 0.0 || d->grip_open == 0.0)
            return fail(c, IRLOSC_ERR_ARG, "policy: grip_close=%g and grip_open=%g must be finite and not 0", d->grip_close, d->grip_open);
    }
    if ((rc = check_rig(c, "policy", nd, d))) return rc;
    if (!weights || !origin) return fail(c, IRLOSC_ERR_ARG, "policy: %s is NULL", !weights ? "weights" : "origin");
    for (size_t i = 0; i < (size_t)d->nb_origin * 6; ++i)
        if (!std::isfinite(origin[i])) return fail(c, IRLOSC_ERR_ARG, "policy: origin of robot %zu is not finite", i / 6);
    const bool looks = (d->obs & IRLOSC_OBS_OBJECT_POSE) != 0;
    if (looks && (!s.objects.count() || s.objects.robots < B))
        return fail(c, IRLOSC_ERR_STATE, "slot %d has no action objects for %d robots, the policy observes them (irlosc_set_objects first)", slot, B);
    const int nobj = looks ? s.objects.count() : -1;
    const int widths[7] = {n, n, nd * 7, nd * 7, nd * 6, 6, std::max(0, nobj) * 7};
    int n_in = 0;
    for (int i = 0; i < 7; ++i) n_in += ((d->obs >> i) & 1u) ? widths[i] : 0;
    if (n_in < 1 || n_in > IRLOSC_POLICY_MAX_IN) return fail(c, IRLOSC_ERR_ARG, "policy: n_in=%d of obs=0x%x out of [1,%d]", n_in, d->obs, IRLOSC_POLICY_MAX_IN);
    size_t nw = 0;
    for (int l = 0, in = n_in; l < L; ++l) { const int o = l < L - 1 ? d->width[l] : d->n_out; nw += (size_t)o * in + o; in = o; }
    for (size_t i = 0; i < nw; ++i)
        if (!std::isfinite(weights[i])) return fail(c, IRLOSC_ERR_ARG, "policy: weight %zu is not finite", i);
    if (!c->model.in_force) return fail(c, IRLOSC_ERR_STATE, "irlosc_set_model has not been called");
    if (B > std::max(0, s.targets))
        return fail(c, IRLOSC_ERR_STATE, "slot %d holds targets for %d instances, policy given for %d: irlosc_set_targets first", slot, std::max(0, s.targets), B);
    HIPCHK(c, hipSetDevice(c->cfg.hip_device));
    Program& p = s.prog;
    p.end();           // (none until the new one is in its buffers; the policy writes the targets from here on: paths, a list or a stream end)
    s.episodes.end();  // (set on the program this call replaces)
    std::vector<float> packed;
    const PolicyNet net = policy_net(*d, n_in, weights, &packed);
    irlosc_teleop_stream rig{};      // the rig in a stream's form: what teleop_args and the shared body read
    rig.ticks = 1; rig.nb = 1; rig.nb_origin = d->nb_origin; rig.increment = d->increment;
    memcpy(rig.kind, d->kind, sizeof rig.kind); memcpy(rig.off_xyz, d->off_xyz, sizeof rig.off_xyz);
    memcpy(rig.off_quat, d->off_quat, sizeof rig.off_quat); memcpy(rig.heading_offset, d->heading_offset, sizeof rig.heading_offset);
    std::vector<double> org;
    if (d->nb_origin > 1) org = walk_table(origin, d->nb_origin, 6);
    const size_t Bm = (size_t)c->cfg.max_batch, out_bytes = 7 * Bm * sizeof(float), obs_bytes = d->keep_obs ? (size_t)B * n_in * sizeof(float) : 0;
    if (!got(p.ts_pose.ensure(p.ts_words(Bm) * sizeof(double))) || !got(p.ts_origin.reserve(org.size() * sizeof(double))) ||
        !got(p.po_w.reserve(packed.size() * sizeof(float))) || !got(p.po_out.ensure(out_bytes)) || !got(p.po_grip.ensure(Bm * sizeof(double))) ||
        !got(p.po_obs.reserve(obs_bytes)))
        return fail(c, IRLOSC_ERR_HIP, "out of device memory for the policy of slot %d", slot);
    const TeleopArgs init = teleop_args(c, s, B, rig, origin, -1);
    const auto launch = c->cfg.dtype == IRLOSC_F64 ? launch_teleop<double> : launch_teleop<float>;
    rc = setter_upload(c, {{p.ts_origin, org.data(), org.size() * sizeof(double)}, {p.po_w, packed.data(), packed.size() * sizeof(float)},
                           {p.po_out, nullptr, out_bytes, 0}, {p.po_grip, nullptr, Bm * sizeof(double), 0}, {p.po_obs, nullptr, obs_bytes, 0}}, launch, &init);
    if (!rc) p.policy(B, *d, rig, net, nobj, origin);
    return rc;
}

extern "C" int irlosc_download_policy_state(irlosc_ctx* c, int32_t slot, int32_t B, double* pose, float* out, double* grip, float* obs, int32_t* tick) {
    if (!c) return IRLOSC_ERR_ARG;
    int rc = check_slot(c, slot, B);
    if (!rc) rc = check_program(c, slot, B, Program::POLICY);
    if (rc) return rc;
    const Program& p = c->slot[slot].prog;
    if (obs && !p.po.keep_obs) return fail(c, IRLOSC_ERR_STATE, "slot %d: its policy keeps no observation (keep_obs == 0)", slot);
    if (tick) *tick = p.tick;
    if (B == 0) return IRLOSC_OK;
    HIPCHK(c, hipSetDevice(c->cfg.hip_device));
    const size_t Bm = (size_t)c->cfg.max_batch, no = (size_t)p.po.n_out;      // rows [max_batch] on the device -> [B][6], [B][n_out], [B] for the caller
    if (obs) HIPCHK(c, hipMemcpyAsync(obs, p.po_obs, (size_t)B * p.po_net.n_in * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    if (pose || out) rc = download_state(c, B, pose ? p.ts_pose.get() : nullptr, pose ? p.ts_words(Bm) : 0, {{pose, p.pose(Bm), 6, 6, 0, 1}},      // (out: float words moved as int32 words)
                                         out ? (const int32_t*)p.po_out.get() : nullptr, out ? no * Bm : 0, {{(int32_t*)out, (const int32_t*)p.po_out.get(), no, no, 0, 1}});
    if (!rc) rc = download_state(c, B, grip ? p.po_grip.get() : nullptr, grip ? Bm : 0, {{grip, p.po_grip.get(), 1, 1, 0, 1}}, nullptr, 0, {});      // (synchronises: obs is in)
    return rc;
}

// ---- the Gaussian head of the policy in force (osc_policy.hpp: the NOISE form; osc_rng.hpp) ---------------------------------------------
extern "C" int irlosc_set_policy_noise(irlosc_ctx* c, int32_t slot, const irlosc_policy_noise* d, const uint32_t* draw0) {
    if (!c) return IRLOSC_ERR_ARG;
    int rc = check_slot(c, slot, 0);
    if (rc) return rc;
    Program& p = c->slot[slot].prog;
    if (!d) { p.exact(); return IRLOSC_OK; }
    if (d->reserved != 0) return fail(c, IRLOSC_ERR_ARG, "policy noise: reserved must be 0");
    if (d->n_std != 6 && d->n_std != 7) return fail(c, IRLOSC_ERR_ARG, "policy noise: n_std=%d must be 6 or 7", d->n_std);
    int m = 0;
    double sum_ln = 0.0;       // C = sum of ln std[c] over the noisy outputs, c ascending, + (m / 2) ln 2 pi
    for (int i = 0; i < 8; ++i) {
        const float sd = d->std[i];
        if (i >= d->n_std) {
            if (sd != 0.0f) return fail(c, IRLOSC_ERR_ARG, "policy noise: std[%d]=%g behind n_std=%d must be 0", i, (double)sd, d->n_std);      // (a NaN is not 0)
            continue;
        }
        if (!std::isfinite(sd) || sd < 0.0f) return fail(c, IRLOSC_ERR_ARG, "policy noise: std[%d]=%g must be finite and >= 0", i, (double)sd);
        if (sd > 0.0f) { ++m; sum_ln += std::log((double)sd); }
    }
    if (!m) return fail(c, IRLOSC_ERR_ARG, "policy noise: every std is 0 (desc == NULL ends a head)");
    if (p.kind != Program::POLICY) return fail(c, IRLOSC_ERR_STATE, "slot %d has no policy (irlosc_set_policy)", slot);
    if (d->n_std != p.po.n_out) return fail(c, IRLOSC_ERR_ARG, "policy noise: n_std=%d, the policy in force has n_out=%d", d->n_std, p.po.n_out);
    const double logp_const = sum_ln + (0.5 * (double)m) * 1.8378770664093453;      // ln 2 pi
    HIPCHK(c, hipSetDevice(c->cfg.hip_device));
    const size_t Bm = (size_t)c->cfg.max_batch, B = (size_t)p.robots, act_bytes = 7 * Bm * sizeof(float);
    p.exact();                 // (none until the new one's state is in its buffers)
    if (!got(p.pn_act.ensure(act_bytes)) || !got(p.pn_logp.ensure(Bm * sizeof(double))) || !got(p.pn_draws.ensure(Bm * sizeof(uint32_t))))
        return fail(c, IRLOSC_ERR_HIP, "out of device memory for the policy noise of slot %d", slot);
    rc = setter_upload(c, {{p.pn_act.get(), nullptr, act_bytes, 0}, {p.pn_logp.get(), nullptr, Bm * sizeof(double), 0},
                           {p.pn_draws.get(), nullptr, Bm * sizeof(uint32_t), 0}, {p.pn_draws.get(), draw0, draw0 ? B * sizeof(uint32_t) : 0, 0}});
    if (!rc) p.samples(*d, logp_const);
    return rc;
}

extern "C" int irlosc_download_policy_noise_state(irlosc_ctx* c, int32_t slot, int32_t B, float* act, double* logp, uint32_t* draws, double* logp_const) {
    if (!c) return IRLOSC_ERR_ARG;
    int rc = check_slot(c, slot, B);
    if (!rc) rc = check_program(c, slot, B, Program::POLICY);
    if (rc) return rc;
    const Program& p = c->slot[slot].prog;
    if (!p.noise) return fail(c, IRLOSC_ERR_STATE, "slot %d: its policy has no Gaussian head (irlosc_set_policy_noise)", slot);
    if (logp_const) *logp_const = p.pn_const;
    if (B == 0) return IRLOSC_OK;
    HIPCHK(c, hipSetDevice(c->cfg.hip_device));
    const size_t Bm = (size_t)c->cfg.max_batch, no = (size_t)p.po.n_out;      // rows [max_batch] on the device -> [B][n_out], [B], [B]
    if (draws) HIPCHK(c, hipMemcpyAsync(draws, p.pn_draws.get(), (size_t)B * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    if (logp) HIPCHK(c, hipMemcpyAsync(logp, p.pn_logp.get(), (size_t)B * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    return download_state(c, B, nullptr, 0, {}, act ? (const int32_t*)p.pn_act.get() : nullptr, act ? no * Bm : 0,      // (act: float words moved as int32 words; synchronises)
                          {{(int32_t*)act, (const int32_t*)p.pn_act.get(), no, no, 0, 1}});
}

extern "C" int irlosc_download_targets(irlosc_ctx* c, int32_t slot, int32_t B, void* tgt_pose) {
    if (!c) return IRLOSC_ERR_ARG;
    int rc = check_slot(c, slot, B);
    if (rc) return rc;
    const Slot& s = c->slot[slot];
    if (!tgt_pose) return fail(c, IRLOSC_ERR_ARG, "tgt_pose is NULL");
    if (B > std::max(0, s.targets))
        return fail(c, IRLOSC_ERR_STATE, "slot %d holds targets for %d instances, asked for %d", slot, std::max(0, s.targets), B);
    if (B == 0) return IRLOSC_OK;
    HIPCHK(c, hipSetDevice(c->cfg.hip_device));
    HIPCHK(c, hipMemcpyAsync(tgt_pose, s.tgt, (size_t)B * c->cfg.ndev * 7 * c->esz, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return IRLOSC_OK;
}

// ---- the reward of the rollout (osc_reward.hpp) ---------------------------------------------------------------------------------------
extern "C" int irlosc_set_reward(irlosc_ctx* c, int32_t slot, int32_t B, const irlosc_reward* d, const double* points) {
    if (!c) return IRLOSC_ERR_ARG;
    int rc = check_slot(c, slot, B);
    if (rc) return rc;
    Slot& s = c->slot[slot];
    if (!d) { s.reward.end(); return IRLOSC_OK; }
    const int nd = c->cfg.ndev, P = d->n_points;
    if (d->n_terms < 1 || d->n_terms > IRLOSC_MAX_REWARD_TERMS) return fail(c, IRLOSC_ERR_ARG, "reward: n_terms=%d out of [1,%d]", d->n_terms, IRLOSC_MAX_REWARD_TERMS);
    if (P < 0 || P > IRLOSC_MAX_REWARD_POINTS) return fail(c, IRLOSC_ERR_ARG, "reward: n_points=%d out of [0,%d]", P, IRLOSC_MAX_REWARD_POINTS);
    if (d->points_per_robot != 0 && d->points_per_robot != 1) return fail(c, IRLOSC_ERR_ARG, "reward: points_per_robot=%d must be 0 or 1", d->points_per_robot);
    if (d->reserved[0] != 0 || d->reserved[1] != 0) return fail(c, IRLOSC_ERR_ARG, "reward: reserved must be 0");
    if (B < 1) return fail(c, IRLOSC_ERR_ARG, "reward: B=%d must be >= 1", B);
    if (!std::isfinite(d->gamma) || d->gamma < 0.0 || d->gamma > 1.0) return fail(c, IRLOSC_ERR_ARG, "reward: gamma=%g must be finite and in [0,1]", d->gamma);
    if (d->goal_term < -1 || d->goal_term >= d->n_terms) return fail(c, IRLOSC_ERR_ARG, "reward: goal_term=%d out of [-1,%d)", d->goal_term, d->n_terms);
    if (d->goal_cmp != 0 && d->goal_cmp != 1) return fail(c, IRLOSC_ERR_ARG, "reward: goal_cmp=%d must be 0 (<=) or 1 (>=)", d->goal_cmp);
    if (d->goal_hold < 1) return fail(c, IRLOSC_ERR_ARG, "reward: goal_hold=%d must be >= 1", d->goal_hold);
    if (!std::isfinite(d->goal_value)) return fail(c, IRLOSC_ERR_ARG, "reward: goal_value is not finite");
    if (P > 0 && !points) return fail(c, IRLOSC_ERR_ARG, "reward: points is NULL with n_points=%d", P);
    // a point (kind, index) of term i; quat: the term reads its orientation
    auto point = [&](int i, const char* which, int kind, int index, bool quat) -> int {
        if (kind < IRLOSC_REWARD_EE || kind > IRLOSC_REWARD_FIXED) return fail(c, IRLOSC_ERR_ARG, "reward: term %d: %s_kind=%d is no point kind", i, which, kind);
        const int lim = kind == IRLOSC_REWARD_OBJECT ? IRLOSC_MAX_OBJECTS : kind == IRLOSC_REWARD_FIXED ? P : nd;
        if (index < 0 || index >= lim) return fail(c, IRLOSC_ERR_ARG, "reward: term %d: %s_index=%d out of [0,%d)", i, which, index, lim);
        if (quat && kind == IRLOSC_REWARD_FIXED) return fail(c, IRLOSC_ERR_ARG, "reward: term %d: ORI on a FIXED point, which has no orientation", i);
        return IRLOSC_OK;
    };
    for (int i = 0; i < IRLOSC_MAX_REWARD_TERMS; ++i) {
        const int kind = d->kind[i];
        if (i >= d->n_terms) {
            if (kind || d->a_kind[i] || d->a_index[i] || d->b_kind[i] || d->b_index[i] || d->weight[i] != 0.0)      // (a NaN is not 0)
                return fail(c, IRLOSC_ERR_ARG, "reward: term %d behind n_terms=%d must be all zero", i, d->n_terms);
            continue;
        }
        if (kind < IRLOSC_REWARD_DIST_SQ || kind > IRLOSC_REWARD_ONE) return fail(c, IRLOSC_ERR_ARG, "reward: term %d: kind=%d is no term kind", i, kind);
        if (!std::isfinite(d->weight[i])) return fail(c, IRLOSC_ERR_ARG, "reward: term %d: its weight is not finite", i);
        if (kind <= IRLOSC_REWARD_ORI) {
            if ((rc = point(i, "a", d->a_kind[i], d->a_index[i], kind == IRLOSC_REWARD_ORI)) || (rc = point(i, "b", d->b_kind[i], d->b_index[i], kind == IRLOSC_REWARD_ORI))) return rc;
            continue;
        }
        const int lim = kind == IRLOSC_REWARD_FORCE ? nd : kind == IRLOSC_REWARD_MATED ? IRLOSC_MAX_MATES : 1;      // what a_index names
        if (d->a_index[i] < 0 || d->a_index[i] >= lim) return fail(c, IRLOSC_ERR_ARG, "reward: term %d: a_index=%d out of [0,%d)", i, d->a_index[i], lim);
        if (d->a_kind[i] || d->b_kind[i] || d->b_index[i]) return fail(c, IRLOSC_ERR_ARG, "reward: term %d (kind %d) reads no point: a_kind, b_kind and b_index must be 0", i, kind);
    }
    const int nbp = d->points_per_robot ? B : 1;
    for (size_t i = 0; i < (size_t)nbp * P * 3; ++i)
        if (!std::isfinite(points[i])) return fail(c, IRLOSC_ERR_ARG, "reward: point %zu of robot %zu is not finite", i / 3 % P, i / 3 / P);
    if ((rc = check_reward_refs(c, slot, B, *d))) return rc;
    if (s.episodes.robots > B)
        return fail(c, IRLOSC_ERR_STATE, "slot %d: its episodes cover %d robots, the reward is given for %d (their resets write its state)", slot, s.episodes.robots, B);
    HIPCHK(c, hipSetDevice(c->cfg.hip_device));
    Reward& w = s.reward;
    w.end();           // (none until the new one's state is fresh)
    const int pr = d->points_per_robot && B > 1 && P > 0;
    const std::vector<double> tab = P > 0 ? walk_table(points, pr ? B : 1, (size_t)P * 3) : std::vector<double>();
    const size_t Bm = (size_t)c->cfg.max_batch;
    const bool first = !w.st_d.get();      // (the first use: the ring starts as zeros; later settings leave it alone)
    if (!got(w.st_d.ensure(w.d_words(Bm) * sizeof(double))) || !got(w.st_i.ensure(w.i_words(Bm) * sizeof(int32_t))) || !got(w.table.reserve(tab.size() * sizeof(double))))
        return fail(c, IRLOSC_ERR_HIP, "out of device memory for the reward of slot %d", slot);
    const RewardArgs init = reward_args(c, s, B, *d, pr, nullptr, nullptr);      // (the init launch: reward_fresh for the B robots)
    rc = setter_upload(c, {{w.table, tab.data(), tab.size() * sizeof(double), 0}, {w.st_d, nullptr, first ? w.d_words(Bm) * sizeof(double) : 0, 0}},
                       c->cfg.dtype == IRLOSC_F64 ? launch_reward<double> : launch_reward<float>, &init);
    if (rc) return rc;
    w.set(B, *d, pr, s.episodes.robots ? s.episodes.serial : -1, s.episodes.tick);
    return IRLOSC_OK;
}

extern "C" int irlosc_download_reward_state(irlosc_ctx* c, int32_t slot, int32_t B, double* r, double* ret, double* gret, int32_t* steps, int32_t* hold,
                                            int32_t* goal_step, double* records) {
    if (!c) return IRLOSC_ERR_ARG;
    int rc = check_slot(c, slot, B);
    if (rc) return rc;
    const Slot& s = c->slot[slot];
    rc = check_covers(c, slot, B, s.reward.robots, "reward", "covers", "irlosc_set_reward");
    if (rc || B == 0) return rc;
    const Reward& w = s.reward;
    const Episodes& e = s.episodes;
    HIPCHK(c, hipSetDevice(c->cfg.hip_device));
    const size_t Bm = (size_t)c->cfg.max_batch, NR = IRLOSC_MAX_EPISODE_RECORDS;      // rows [max_batch] on the device -> [B], [B][NR][2] for the caller
    const RewardState st = w.state(Bm);
    rc = download_state(c, B, w.st_d, w.d_words(Bm), {{r, st.r, 1, 1, 0, 1}, {ret, st.ret, 1, 1, 0, 1}, {gret, st.gret, 1, 1, 0, 1}, {records, st.ring, 2 * NR, 2 * NR, 0, 1}},
                        w.st_i, w.i_words(Bm), {{steps, st.steps, 1, 1, 0, 1}, {hold, st.hold, 1, 1, 0, 1}, {goal_step, st.goal_step, 1, 1, 0, 1}});
    if (rc || !records) return rc;
    // the mask: an entry counts when an episode of the running count, ended under this reward, wrote it -- the episodes were set behind the
    // reward (every entry below count), or the episode ended on a tick of theirs not before the reward came in force
    // (per robot: the episodes may cover fewer robots than this download -- the others' entries are zero)
    const int Be = std::min(B, e.robots);
    std::vector<int32_t> cnt((size_t)B, 0), ring(Be ? (size_t)Be * 4 * e.d.records : 0);
    if (Be) {
        rc = download_state(c, Be, nullptr, 0, {}, e.st_i, e.i_words(Bm), {{cnt.data(), e.count(Bm), 1, 1, 0, 1}, {ring.data(), e.ring(Bm), 4 * (size_t)e.d.records, 4 * (size_t)e.d.records, 0, 1}});
        if (rc) return rc;
    }
    for (size_t b = 0; b < (size_t)B; ++b)
        for (size_t k = 0; k < NR; ++k) {
            bool ok = (int)b < Be && (int)k < e.d.records && (int)k < cnt[b];
            if (ok && e.serial == w.ep_serial) {
                const int32_t* rec = &ring[(b * e.d.records + k) * 4];
                ok = rec[0] + rec[1] - 1 >= w.ep_tick0;      // (start_tick + length - 1: the episodes' tick it ended on)
            }
            if (!ok) records[(b * NR + k) * 2] = records[(b * NR + k) * 2 + 1] = 0.0;
        }
    return IRLOSC_OK;
}

// ---- episodes of the rollout (osc_episode.hpp) --------------------------------------------------------------------------------------
extern "C" int irlosc_set_episodes(irlosc_ctx* c, int32_t slot, int32_t B, const irlosc_episodes* d, const double* qpos0, const double* qvel0,
                                   const double* poses) {
    if (!c) return IRLOSC_ERR_ARG;
    int rc = check_slot(c, slot, B);
    if (rc) return rc;
    Slot& s = c->slot[slot];
    if (!d) { s.episodes.end(); return IRLOSC_OK; }
    const int n = c->cfg.n, nd = c->cfg.ndev, S = d->n_starts, V = d->n_variants;
    if (d->max_ticks < 0 || d->max_episodes < 0 || d->poll_every < 0)
        return fail(c, IRLOSC_ERR_ARG, "episodes: max_ticks=%d, max_episodes=%d, poll_every=%d must be >= 0", d->max_ticks, d->max_episodes, d->poll_every);
    if ((d->end_on_finish != 0 && d->end_on_finish != 1) || (d->starts_per_robot != 0 && d->starts_per_robot != 1))
        return fail(c, IRLOSC_ERR_ARG, "episodes: end_on_finish=%d, starts_per_robot=%d must be 0 or 1", d->end_on_finish, d->starts_per_robot);
    if (S < 1 || S > IRLOSC_MAX_EPISODE_STARTS) return fail(c, IRLOSC_ERR_ARG, "episodes: n_starts=%d out of [1,%d]", S, IRLOSC_MAX_EPISODE_STARTS);
    if (V < 0 || V > IRLOSC_MAX_EPISODE_STARTS) return fail(c, IRLOSC_ERR_ARG, "episodes: n_variants=%d out of [0,%d]", V, IRLOSC_MAX_EPISODE_STARTS);
    if (d->records < 1 || d->records > IRLOSC_MAX_EPISODE_RECORDS)
        return fail(c, IRLOSC_ERR_ARG, "episodes: records=%d out of [1,%d]", d->records, IRLOSC_MAX_EPISODE_RECORDS);
    if (d->reserved != 0) return fail(c, IRLOSC_ERR_ARG, "episodes: reserved must be 0");
    if (B < 1) return fail(c, IRLOSC_ERR_ARG, "episodes: B=%d must be >= 1", B);
    if (!qpos0 || !qvel0) return fail(c, IRLOSC_ERR_ARG, "episodes: qpos0 and qvel0 are required");
    if (V > 0 && !poses) return fail(c, IRLOSC_ERR_ARG, "episodes: poses is NULL with n_variants=%d", V);
    const int nbs = d->starts_per_robot ? B : 1;
    for (size_t i = 0; i < (size_t)nbs * S * n; ++i)
        if (!std::isfinite(qpos0[i]) || !std::isfinite(qvel0[i]))
            return fail(c, IRLOSC_ERR_ARG, "episodes: start state %zu of robot %zu is not finite", i / n % S, i / n / S);
    if (!c->model.in_force) return fail(c, IRLOSC_ERR_STATE, "irlosc_set_model has not been called");
    if (n != plant_joints()) return fail(c, IRLOSC_ERR_STATE, "no episodes on this context: the rollout's kernels hold %d joints, n=%d", plant_joints(), n);
    if (B > std::max(0, s.targets))
        return fail(c, IRLOSC_ERR_STATE, "slot %d holds targets for %d instances, episodes given for %d: irlosc_set_targets first", slot,
                    std::max(0, s.targets), B);
    const Program& p = s.prog;
    for (const Slot::Cover& k : s.reset_covers())
        if (k.robots && B > k.robots)
            return fail(c, IRLOSC_ERR_STATE, "slot %d: its %s covers %d robots, episodes given for %d (their resets write its state)", slot, k.what, k.robots, B);
    if (p.kind == Program::STREAM)
        return fail(c, IRLOSC_ERR_STATE, "slot %d has a teleoperation stream: its reading index is the slot's tick, not a robot's (no episodes next to it)", slot);
    if (s.push.robots)
        return fail(c, IRLOSC_ERR_STATE, "slot %d has pushes: their windows are the slot's ticks, not a robot's (no episodes next to them)", slot);
    const int A = p.kind == Program::LIST ? p.al.n_actions : 0;
    if (V > 0 && p.kind != Program::LIST) return fail(c, IRLOSC_ERR_STATE, "episodes: pose variants need an action list on slot %d (irlosc_set_action_list)", slot);
    if (V > 0 && p.al.nb == 1 && p.robots > 1)
        return fail(c, IRLOSC_ERR_STATE, "episodes: pose variants need a pose table per robot, the list of slot %d shares one (nb == 1)", slot);
    for (size_t i = 0; i < (size_t)V * B * A; ++i)
        for (int w = 0; w < 7 && p.al.kind[i % A] == IRLOSC_ACTION_WP; ++w)
            if (!std::isfinite(poses[i * 7 + w]))
                return fail(c, IRLOSC_ERR_ARG, "episodes: pose of action %zu, robot %zu, variant %zu is not finite", i % A, i / A % B, i / A / B);
    HIPCHK(c, hipSetDevice(c->cfg.hip_device));
    Episodes& e = s.episodes;
    e.end();           // (none until the new ones are in their buffers and their state is reset)
    // the start states, a hinge's pair side by side as the walk's layout has them; the variants, each laid out as the list's own table
    std::vector<double> dense((size_t)nbs * S * 2 * n);
    for (size_t i = 0; i < (size_t)nbs * S; ++i)
        for (int j = 0; j < n; ++j) { dense[(i * n + j) * 2] = qpos0[i * n + j]; dense[(i * n + j) * 2 + 1] = qvel0[i * n + j]; }
    const int starts_pr = d->starts_per_robot && B > 1, list_pr = V > 0 && p.al.nb > 1;
    const std::vector<double> st = walk_table(dense.data(), starts_pr ? B : 1, (size_t)S * 2 * n);
    const size_t E = (size_t)A * 7, vstride = list_pr ? ((size_t)B + 63) / 64 * E * 64 : E;
    std::vector<double> vt((size_t)V * vstride, 0.0);
    for (size_t v = 0; v < (size_t)V; ++v)
        for (size_t b = 0; b < (size_t)B; ++b)
            for (size_t k = 0; k < E; ++k) vt[v * vstride + (list_pr ? ((b / 64) * E + k) * 64 + b % 64 : k)] = poses[(v * B + b) * E + k];
    const size_t Bm = (size_t)c->cfg.max_batch, i_bytes = e.i_words(Bm) * sizeof(int32_t);
    if (!got(e.st_i.ensure(i_bytes)) || !got(e.running.ensure((Bm + 63) / 64 * sizeof(int32_t))) || !got(e.snap.ensure(Bm * nd * 7 * c->esz)) ||
        !got(e.starts.reserve(st.size() * sizeof(double))) || !got(e.variants.reserve(vt.size() * sizeof(double))) || !got(s.qt.ensure(qt_bytes(c))))
        return fail(c, IRLOSC_ERR_HIP, "out of device memory for the episodes of slot %d", slot);
    e.laid_out(starts_pr, list_pr, vstride);
    const EpisodeArgs init = episode_args(c, s, B, *d, true);
    rc = setter_upload(c, {{e.starts, st.data(), st.size() * sizeof(double)}, {e.variants, vt.data(), vt.size() * sizeof(double)},
                           {e.st_i, nullptr, i_bytes, 0}},      // (the ring = 0; count, age, start_tick: the init launch)
                       c->cfg.dtype == IRLOSC_F64 ? launch_episodes<double> : launch_episodes<float>, &init);
    if (rc) return rc;
    e.set(B, *d);
    s.restarted(B);
    return IRLOSC_OK;
}

extern "C" int irlosc_download_episode_state(irlosc_ctx* c, int32_t slot, int32_t B, int32_t* count, int32_t* age, int32_t* start_tick,
                                             int32_t* running, int32_t* records, int32_t* ticks_run) {
    if (!c) return IRLOSC_ERR_ARG;
    int rc = check_slot(c, slot, B);
    if (rc) return rc;
    const Slot& s = c->slot[slot];
    if (ticks_run) *ticks_run = s.ticks_run;
    if (B == 0) return IRLOSC_OK;
    rc = check_covers(c, slot, B, s.episodes.robots, "episodes", "cover", "irlosc_set_episodes");
    if (rc) return rc;
    const Episodes& e = s.episodes;
    HIPCHK(c, hipSetDevice(c->cfg.hip_device));
    const size_t Bm = (size_t)c->cfg.max_batch, R = (size_t)e.d.records;      // rows [max_batch] on the device -> [B], [B][R][4] for the caller
    std::vector<int32_t> cnt((size_t)B);
    rc = download_state(c, B, nullptr, 0, {}, e.st_i, e.i_words(Bm), {{cnt.data(), e.count(Bm), 1, 1, 0, 1}, {age, e.age(Bm), 1, 1, 0, 1},
                        {start_tick, e.start_tick(Bm), 1, 1, 0, 1}, {records, e.ring(Bm), 4 * R, 4 * R, 0, 1}});
    if (rc) return rc;
    int live = 0;
    for (int b = 0; b < B; ++b) {
        if (count) count[b] = cnt[b];
        live += !(e.d.max_episodes > 0 && cnt[b] >= e.d.max_episodes);
    }
    if (running) *running = live;
    return IRLOSC_OK;
}

extern "C" int irlosc_device_sync(irlosc_ctx* c) {
    if (!c) return IRLOSC_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->cfg.hip_device));
    HIPCHK(c, hipDeviceSynchronize());
    return IRLOSC_OK;
}

extern "C" int irlosc_tick(irlosc_ctx* c, int32_t B, const void* M, const void* J, const void* dq, const void* bias,
                           const void* ee_pose, const void* wrench, const void* tgt_pose, const void* tgt_vel, void* u_host,
                           uint32_t* flags_host) {
    if (!c) return IRLOSC_ERR_ARG;
    if (B < 0 || B > c->cfg.max_batch) return fail(c, IRLOSC_ERR_ARG, "B=%d out of [0,%d]", B, c->cfg.max_batch);
    if (B == 0) return IRLOSC_OK;
    if (!M || !J || !dq || !ee_pose || !tgt_pose || !u_host) return fail(c, IRLOSC_ERR_ARG, "M, J, dq, ee_pose, tgt_pose and u_host are required");
    if ((c->cfg.flags & IRLOSC_USE_G) && !bias) return fail(c, IRLOSC_ERR_ARG, "bias required with IRLOSC_USE_G");
    if (c->gains_nb == 0) return fail(c, IRLOSC_ERR_STATE, "irlosc_set_gains has not been called");
    HIPCHK(c, hipSetDevice(c->cfg.hip_device));
    const size_t b = (size_t)B, n = (size_t)c->cfg.n, k = (size_t)c->k, nd = (size_t)c->cfg.ndev, e = c->esz;
    // input block: M | J | dq | bias | ee | tgt | wrench | tvel, each piece 256-byte aligned
    const void* src[8] = {M, J, dq, bias, ee_pose, tgt_pose, wrench, tgt_vel};
    const size_t sz[8] = {b * n * n * e, b * k * n * e, b * n * e, bias ? b * n * e : 0, b * nd * 7 * e, b * nd * 7 * e,
                          wrench ? b * nd * 6 * e : 0, tgt_vel ? b * nd * 6 * e : 0};
    size_t off[8], total = 0;
    for (int i = 0; i < 8; ++i) { off[i] = total; total += (sz[i] + 255) & ~(size_t)255; }
    HIPCHK(c, c->tick_hin.reserve(total));
    HIPCHK(c, c->tick_din.reserve(total));
    // output block: u | flags | the two words of the symmetry probe (they ride back in the one copy the tick makes anyway)
    const size_t ub = b * n * e, fl_off = (ub + 255) & ~(size_t)255, sym_off = (fl_off + b * sizeof(uint32_t) + 15) & ~(size_t)15;
    const size_t out_total = sym_off + 2 * sizeof(int32_t);
    const bool sym_dev = sym_applies(c) && B > SYM_HOST_MAX_B;
    if (sym_applies(c) && !sym_dev) {
        int rch = symmetry_host(c, M, B);
        if (rch) return rch;
    }
    HIPCHK(c, c->tick_hout.reserve(out_total));
    HIPCHK(c, c->tick_dout.reserve(out_total));
    unsigned char* hin = c->tick_hin;
    unsigned char* din = c->tick_din;
    for (int i = 0; i < 8; ++i) if (sz[i]) memcpy(hin + off[i], src[i], sz[i]);
    HIPCHK(c, hipMemcpyAsync(din, hin, total, hipMemcpyHostToDevice, c->stream));
    unsigned char* dout = c->tick_dout;
    uint32_t* dfl = (uint32_t*)(dout + fl_off);
    if (sym_dev) {
        int rcs = symmetry_probe(c, din + off[0], B, (int32_t*)(dout + sym_off), c->stream);
        if (rcs) return rcs;
    }
    int rc = launch(c, B, StepInputs{din + off[0], din + off[1], din + off[2], sz[3] ? din + off[3] : nullptr, din + off[4], din + off[5],
                                     sz[7] ? din + off[7] : nullptr, sz[6] ? din + off[6] : nullptr}, dout, dfl, c->stream);
    if (rc) return rc;
    unsigned char* hout = c->tick_hout;
    HIPCHK(c, hipMemcpyAsync(hout, dout, out_total, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (sym_dev) {                                      // nothing is handed out for an asymmetric M
        int rcs = symmetry_verdict(c, (const int32_t*)(hout + sym_off));
        if (rcs) return rcs;
    }
    memcpy(u_host, hout, ub);
    if (flags_host) memcpy(flags_host, hout + fl_off, b * sizeof(uint32_t));
    return IRLOSC_OK;
}

// ---- multi-GPU throughput reduction over RCCL (dlopen: a single-GPU deployment never loads librccl) ---------------
namespace {
struct RcclApi {
    void* h = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*AllGather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    const char* (*GetErrorString)(ncclResult_t) = nullptr;
};
RcclApi g_rccl;
thread_local std::string g_comm_error;

int comm_fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_comm_error = buf;
    return code;
}

int rccl_load() {
    if (g_rccl.h) return IRLOSC_OK;
    void* h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
    if (!h) h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!h) h = dlopen("/opt/rocm/lib/librccl.so", RTLD_NOW | RTLD_GLOBAL);
    if (!h) return comm_fail(IRLOSC_ERR_HIP, "cannot load librccl.so: %s", dlerror());
    RcclApi a;
    a.h = h;
    a.GetUniqueId = (decltype(a.GetUniqueId))dlsym(h, "ncclGetUniqueId");
    a.CommInitRank = (decltype(a.CommInitRank))dlsym(h, "ncclCommInitRank");
    a.CommDestroy = (decltype(a.CommDestroy))dlsym(h, "ncclCommDestroy");
    a.AllReduce = (decltype(a.AllReduce))dlsym(h, "ncclAllReduce");
    a.AllGather = (decltype(a.AllGather))dlsym(h, "ncclAllGather");
    a.GetErrorString = (decltype(a.GetErrorString))dlsym(h, "ncclGetErrorString");
    if (!a.GetUniqueId || !a.CommInitRank || !a.CommDestroy || !a.AllReduce || !a.AllGather || !a.GetErrorString)
        return comm_fail(IRLOSC_ERR_HIP, "librccl.so lacks an expected symbol");
    g_rccl = a;
    return IRLOSC_OK;
}
}  // namespace

struct irlosc_comm {
    int device = 0, rank = 0, world = 1;
    ncclComm_t comm = nullptr;
    Stream stream;
    DevBuf<double> dbuf;             // 2 doubles in, 2 doubles out, then `world` uint64 for the all-gather
    std::string err;
};

#define COMMCHK(cm, expr)                                                                                     \
    do {                                                                                                      \
        hipError_t e_ = (expr);                                                                               \
        if (e_ != hipSuccess) {                                                                               \
            int rc_ = comm_fail(IRLOSC_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_));               \
            if (cm) (cm)->err = g_comm_error;                                                                 \
            return rc_;                                                                                       \
        }                                                                                                     \
    } while (0)
#define NCCLCHK(cm, expr)                                                                                     \
    do {                                                                                                      \
        ncclResult_t r_ = (expr);                                                                             \
        if (r_ != ncclSuccess) {                                                                              \
            int rc_ = comm_fail(IRLOSC_ERR_HIP, "%s failed: %s", #expr, g_rccl.GetErrorString(r_));           \
            if (cm) (cm)->err = g_comm_error;                                                                 \
            return rc_;                                                                                       \
        }                                                                                                     \
    } while (0)

extern "C" const char* irlosc_comm_last_error(const irlosc_comm* cm) { return cm ? cm->err.c_str() : g_comm_error.c_str(); }

extern "C" int irlosc_comm_unique_id(uint8_t id_out[IRLOSC_COMM_ID_BYTES]) {
    static_assert(sizeof(ncclUniqueId) == IRLOSC_COMM_ID_BYTES, "unique id size");
    if (!id_out) return comm_fail(IRLOSC_ERR_ARG, "id_out is NULL");
    int rc = rccl_load();
    if (rc) return rc;
    ncclUniqueId id;
    NCCLCHK((irlosc_comm*)nullptr, g_rccl.GetUniqueId(&id));
    memcpy(id_out, &id, sizeof id);
    return IRLOSC_OK;
}

extern "C" int irlosc_comm_create(int32_t hip_device, int32_t rank, int32_t world, const uint8_t id[IRLOSC_COMM_ID_BYTES],
                                  irlosc_comm** out) {
    if (!out) return comm_fail(IRLOSC_ERR_ARG, "out is NULL");
    *out = nullptr;
    if (!id) return comm_fail(IRLOSC_ERR_ARG, "id is NULL");
    if (world < 1 || rank < 0 || rank >= world) return comm_fail(IRLOSC_ERR_ARG, "rank %d outside world of %d", rank, world);
    int ndevs = 0;
    if (hipGetDeviceCount(&ndevs) != hipSuccess || ndevs < 1) return comm_fail(IRLOSC_ERR_HIP, "no HIP device available");
    if (hip_device < 0 || hip_device >= ndevs) return comm_fail(IRLOSC_ERR_ARG, "hip_device=%d but %d device(s) visible", hip_device, ndevs);
    int rc = rccl_load();
    if (rc) return rc;
    irlosc_comm* cm = new (std::nothrow) irlosc_comm();
    if (!cm) return comm_fail(IRLOSC_ERR_HIP, "out of host memory");
    cm->device = hip_device; cm->rank = rank; cm->world = world;
    auto body = [&]() -> int {
        COMMCHK(cm, hipSetDevice(hip_device));
        COMMCHK(cm, cm->stream.ensure());
        COMMCHK(cm, cm->dbuf.ensure((4 + (size_t)world + 1) * sizeof(double)));
        ncclUniqueId uid;
        memcpy(&uid, id, sizeof uid);
        NCCLCHK(cm, g_rccl.CommInitRank(&cm->comm, world, uid, rank));
        return IRLOSC_OK;
    };
    rc = body();
    if (rc) { irlosc_comm_destroy(cm); return rc; }
    *out = cm;
    return IRLOSC_OK;
}

extern "C" void irlosc_comm_destroy(irlosc_comm* cm) {
    if (!cm) return;
    (void)hipSetDevice(cm->device);
    if (cm->stream) (void)hipStreamSynchronize(cm->stream);
    if (cm->comm && g_rccl.CommDestroy) (void)g_rccl.CommDestroy(cm->comm);
    delete cm;      // (the buffer, then the stream)
}

extern "C" int irlosc_bench_allreduce(irlosc_comm* cm, double* steps_sum, double* elapsed_max) {
    if (!cm || !steps_sum || !elapsed_max) return comm_fail(IRLOSC_ERR_ARG, "NULL argument");
    COMMCHK(cm, hipSetDevice(cm->device));
    const double in[2] = {*steps_sum, *elapsed_max};
    COMMCHK(cm, hipMemcpyAsync(cm->dbuf, in, sizeof in, hipMemcpyHostToDevice, cm->stream));
    NCCLCHK(cm, g_rccl.AllReduce(cm->dbuf, cm->dbuf + 2, 1, ncclFloat64, ncclSum, cm->comm, cm->stream));
    NCCLCHK(cm, g_rccl.AllReduce(cm->dbuf + 1, cm->dbuf + 3, 1, ncclFloat64, ncclMax, cm->comm, cm->stream));
    double outv[2];
    COMMCHK(cm, hipMemcpyAsync(outv, cm->dbuf + 2, sizeof outv, hipMemcpyDeviceToHost, cm->stream));
    COMMCHK(cm, hipStreamSynchronize(cm->stream));
    *steps_sum = outv[0];
    *elapsed_max = outv[1];
    return IRLOSC_OK;
}

extern "C" int irlosc_comm_allgather_u64(irlosc_comm* cm, uint64_t mine, uint64_t* all) {
    if (!cm || !all) return comm_fail(IRLOSC_ERR_ARG, "NULL argument");
    COMMCHK(cm, hipSetDevice(cm->device));
    uint64_t* d = (uint64_t*)(cm->dbuf + 4);
    COMMCHK(cm, hipMemcpyAsync(d + cm->world, &mine, sizeof mine, hipMemcpyHostToDevice, cm->stream));
    NCCLCHK(cm, g_rccl.AllGather(d + cm->world, d, 1, ncclUint64, cm->comm, cm->stream));
    COMMCHK(cm, hipMemcpyAsync(all, d, (size_t)cm->world * sizeof(uint64_t), hipMemcpyDeviceToHost, cm->stream));
    COMMCHK(cm, hipStreamSynchronize(cm->stream));
    return IRLOSC_OK;
}

extern "C" int irlosc_step_device(irlosc_ctx* c, int32_t B, const void* dM, const void* dJ, const void* ddq,
                                  const void* dbias, const void* dee_pose, const void* dtgt_pose,
                                  const void* dtgt_vel, const void* dwrench, void* du, uint32_t* dflags,
                                  void* hip_stream) {
    if (!c) return IRLOSC_ERR_ARG;
    if (B < 0 || B > c->cfg.max_batch) return fail(c, IRLOSC_ERR_ARG, "B=%d out of [0,%d]", B, c->cfg.max_batch);
    if (!dM || !dJ || !ddq || !dee_pose || !dtgt_pose || !du || !dflags)
        return fail(c, IRLOSC_ERR_ARG, "dM, dJ, ddq, dee_pose, dtgt_pose, du and dflags are required");
    if ((c->cfg.flags & IRLOSC_USE_G) && !dbias) return fail(c, IRLOSC_ERR_ARG, "dbias required with IRLOSC_USE_G");
    HIPCHK(c, hipSetDevice(c->cfg.hip_device));
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : c->stream;
    return launch(c, B, StepInputs{dM, dJ, ddq, dbias, dee_pose, dtgt_pose, dtgt_vel, dwrench}, du, dflags, st);
}
