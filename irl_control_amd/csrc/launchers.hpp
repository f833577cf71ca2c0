// Host-side launch functions of the kernels, one translation unit per kernel family (tu_*.hip) so that the library builds
// in parallel and a change to one kernel recompiles one unit.  irlosc.hip (the C ABI) only sees these declarations.
#pragma once
#include <hip/hip_runtime.h>

#include "osc_common.hpp"

namespace irlosc {

// tu_generic.hip -- one wavefront per instance (osc_generic.hpp); T = float, double
template <typename T>
int launch_generic(const KParams<T>& p, int blocks, hipStream_t st);

// tu_row16_f64.hip / tu_row16_f32.hip (body: tu_row16_impl.hpp) -- fp64-arithmetic row16 path (osc_row16.hpp); TIN = record type
template <typename TIN> struct Row16Train;
template <typename TIN>
int launch_row16(const Row16Train<TIN>& tr, int nsteps, bool tree, hipStream_t st);      // tree: tree-structured factorisation
void row16_tree_masks(uint32_t mrow[32], uint32_t* jcols);      // zero pattern the tree form relies on (osc_row16.hpp)
// the task pass (part 1 of the task signal as rows of the exchange buffer), then the row16 FROMQ kernel
template <typename TIN>
int launch_row16_fromq(const Row16Train<TIN>& tr, int nsteps, hipStream_t st);
template <typename TIN>
int launch_row16_worklist(const Row16Train<TIN>& tr, int nsteps, int32_t* reset, hipStream_t st);
// tu_row16_pad_{dense,tree,fromq}_{f64,f32}.hip -- the KMAX-padded variants launch_row16 / launch_row16_fromq fall through to for the
// layouts without an instantiation of their own (explicit specialisations, one translation unit each)
template <typename TIN> int launch_row16_pad_dense(const Row16Train<TIN>& tr, int nsteps, hipStream_t st);
template <typename TIN> int launch_row16_pad_tree(const Row16Train<TIN>& tr, int nsteps, hipStream_t st);
template <typename TIN> int launch_row16_pad_fromq(const Row16Train<TIN>& tr, int nsteps, hipStream_t st);
template <> int launch_row16_pad_dense<double>(const Row16Train<double>&, int, hipStream_t);
template <> int launch_row16_pad_dense<float>(const Row16Train<float>&, int, hipStream_t);
template <> int launch_row16_pad_tree<double>(const Row16Train<double>&, int, hipStream_t);
template <> int launch_row16_pad_tree<float>(const Row16Train<float>&, int, hipStream_t);
template <> int launch_row16_pad_fromq<double>(const Row16Train<double>&, int, hipStream_t);
template <> int launch_row16_pad_fromq<float>(const Row16Train<float>&, int, hipStream_t);

// tu_lane_f64.hip / tu_lane_f32.hip -- the OSC step of the fused path in lane-per-robot form + its eigen pass (osc_lane.hpp).
// tier: 0 = rows per end-effector body (stand, right, left) up to (1, 6, 6), 1 = up to (1, 3, 3)
namespace lane { struct LaneTrain; struct RowMap; }
struct FeModel;
int lane_plan(const FeModel& h, lane::RowMap* map);      // -> tier, or -1: no instantiation for this layout
template <typename TIN>
int launch_lane_osc(const Row16Train<TIN>& tr, const lane::LaneTrain& lt, int nsteps, int tier, int eig_blocks, int lane_min, hipStream_t st);
template <> int launch_lane_osc<double>(const Row16Train<double>&, const lane::LaneTrain&, int, int, int, int, hipStream_t);
template <> int launch_lane_osc<float>(const Row16Train<float>&, const lane::LaneTrain&, int, int, int, int, hipStream_t);

// tu_frontend.hip / tu_frontend_lane.hip -- rigid-body front end (osc_frontend.hpp, osc_frontend_lane.hpp); TOUT = record type
struct FeModel;
template <typename TOUT> struct FeOut;
template <typename TOUT>
int launch_frontend_generic(const FeModel* dmodel, const double* qpos, const double* qvel, const FeOut<TOUT>& out, int B, size_t smem,
                            hipStream_t st);
template <typename TOUT>
int launch_frontend_lane_dual_ur5(const FeModel* dmodel, const double* qpos, const double* qvel, const FeOut<TOUT>& out, int B,
                                  double* side, hipStream_t st);
template <typename TOUT> struct FeGenericArgs;
template <typename TOUT>
int launch_frontend_generic_lists(const FeModel* dmodel, const FeGenericArgs<TOUT>& a, int nsteps, size_t smem, hipStream_t st);
// compact form for the fused path: a train of up to FE_TRAIN steps, nothing but the exchange buffer is written
struct FeLaneTrain;
struct FeCompactTables;
int launch_frontend_lane_compact_dual_ur5(const FeModel* dmodel, const FeLaneTrain& tr, int nsteps, hipStream_t st);
// tu_frontend_lane_compact_s.hip -- the same walk with the structural constants of the Dual-UR5's MJCF compiled in (TopoDualUr5S)
int launch_frontend_lane_compact_dual_ur5_s(const FeModel* dmodel, const FeLaneTrain& tr, int nsteps, hipStream_t st);
bool frontend_lane_dual_ur5_s_matches(const FeModel& h);
int launch_q_layout(const double* qpos, const double* qvel, double* qt, int B, int nj, hipStream_t st);      // [wave][2 nj][64]: the fused walk's input layout
void frontend_lane_dual_ur5_tables(const FeModel& h, FeCompactTables* t);
size_t frontend_lane_dual_ur5_side_doubles_per_wave();
bool frontend_lane_dual_ur5_matches(const FeModel& h);

// tu_ft.hip -- the wrench of the F/T sensor feed (osc_ft.hpp): one launch per train, blockIdx.y = step with a feed; T = record type
struct FtTrain;
template <typename T>
int launch_ft_wrench(const FtTrain& tr, int nsteps, hipStream_t st);

// tu_pack.hip -- dense records of a slot -> the compact block of the lane-per-robot OSC step (osc_pack.hpp)
struct PackTable;
struct PackArgs;
bool pack_plan(const FeModel& h, PackTable* t);         // -> false: the layout has no pack (then the slots keep the row16 route)
int pack_entries();                                     // entries per robot of the compact block (FeTopo<TopoDualUr5>::n_compact)
int launch_pack(const PackArgs& a, hipStream_t st);
int launch_span_end(unsigned long long* span, hipStream_t st);      // atomicMax(span + 1, wall clock) behind what the stream holds

// tu_plant.hip -- the plant kernel behind a tick of irlosc_rollout_from_q (osc_plant.hpp): one lane per robot on the compiled Dual-UR5
// tree; T = record type (of u)
struct PlantArgs;
template <typename T>
int launch_plant(const PlantArgs& a, hipStream_t st);
int plant_joints();                                     // hinges of the tree the kernel is compiled for

// tu_waypoint.hip -- the waypoint cycler between the give-up pass and the plant of a rollout tick whose slot has paths
// (osc_waypoint.hpp); T = record type (of the targets)
struct WaypointArgs;
template <typename T>
int launch_waypoints(const WaypointArgs& a, hipStream_t st);

// tu_action.hip -- the WP / GRIP action list between the walk and the first OSC kernel of a rollout tick whose slot has one
// (osc_action.hpp); T = record type (of the targets and of the slot's gain copy)
struct ActionArgs;
template <typename T>
int launch_actions(const ActionArgs& a, hipStream_t st);
// ... the same tick of a slot whose list has a motion (irlosc_set_action_motion): the kernel's MOTION instantiation
struct ActionMotionArgs;
template <typename T>
int launch_actions_motion(const ActionMotionArgs& a, hipStream_t st);

// tu_object.hip -- the action objects of a rollout tick whose slot has some (osc_object.hpp): behind the walk and the SENSE launches,
// directly in front of the action kernel; init mode: the launch of irlosc_set_objects
struct ObjectArgs;
int launch_objects(const ObjectArgs& a, hipStream_t st);

// tu_teleop.hip -- the teleoperation stream where the action list's kernel goes, on a rollout tick whose slot has one and a reading
// for the tick (osc_teleop.hpp); T = record type (of the targets)
struct TeleopArgs;
template <typename T>
int launch_teleop(const TeleopArgs& a, hipStream_t st);

// tu_policy.hip -- the policy where the stream's kernel goes, on a rollout tick whose slot has one (osc_policy.hpp): the observation
// gathered, the network on the f32-input MFMA, the stream's body on its output; T = record type (of the targets and the wrench)
struct PolicyArgs;
template <typename T>
int launch_policy(const PolicyArgs& a, hipStream_t st);

// tu_push.hip -- the external pushes of a rollout tick whose slot has some active (osc_push.hpp): sense mode between the sensor feed's
// wrench kernel and the first kernel that reads the wrench, apply mode in front of the plant; T = record type (of the wrench)
struct PushArgs;
template <typename T>
int launch_pushes(const PushArgs& a, hipStream_t st);

// tu_wall.hip -- the compliant walls of a rollout tick whose slot has some (osc_wall.hpp): sense mode behind the pushes' sense launch,
// apply mode behind the pushes' apply launch, in front of the plant; T = record type (of the wrench)
struct WallArgs;
template <typename T>
int launch_walls(const WallArgs& a, hipStream_t st);

// tu_object_load.hip -- the weight of the objects a slot's grippers carry, on a rollout tick whose slot has loads
// (osc_object_load.hpp): sense mode behind the walls' sense launch, in front of the object kernel; apply mode behind the walls' apply
// launch, in front of the joint rows; T = record type (of the wrench)
struct ObjectLoadArgs;
template <typename T>
int launch_object_loads(const ObjectLoadArgs& a, hipStream_t st);

// tu_joint.hip -- the joint rows of a rollout tick whose slot has some (osc_joint.hpp): range stops, finger couplings and gripper
// drives as one torque per hinge, taken off the bias behind the walls' apply launch, directly in front of the plant
struct JointArgs;
int launch_joints(const JointArgs& a, hipStream_t st);

// tu_reward.hip -- the reward of a rollout tick whose slot has one (osc_reward.hpp): behind the give-up pass, directly in front of the
// log's front launch; init mode: the launch of irlosc_set_reward; T = record type (of u, the targets and the wrench)
struct RewardArgs;
template <typename T>
int launch_reward(const RewardArgs& a, hipStream_t st);

// tu_log.hip -- the episode log of a logged rollout tick (osc_log.hpp): the front launch behind the give-up pass, the back launch (the
// walls' and rows' planes) directly in front of the plant; T = record type (of u, the targets and the wrench)
struct LogArgs;
template <typename T>
int launch_log(const LogArgs& a, hipStream_t st);

// tu_episode.hip -- the episodes of a rollout tick whose slot has some (osc_episode.hpp): behind the plant, the last launch of the tick;
// init mode: the launch of irlosc_set_episodes; T = record type (of the targets and of the gains)
struct EpisodeArgs;
template <typename T>
int launch_episodes(const EpisodeArgs& a, hipStream_t st);

// tu_assemble.hip -- state assembly from raw simulator arrays (osc_assemble.hpp)
struct RawDesc;
template <typename T> struct RawPtrs;
template <typename T>
int launch_assemble(const RawDesc& d, const RawPtrs<T>& r, int B, hipStream_t st);
// out[0] += instances whose M is not symmetric, out[1] = min(out[1], first such instance)
template <typename T>
int launch_symmetry_probe(const T* M, int n, int B, int32_t* out, hipStream_t st);
// out[0] += instances with a non-zero where the masks say zero (M[j][c] outside mrow[j], a column of J outside jcols)
template <typename T>
int launch_structure_probe(const T* M, const T* J, int n, int k, int B, const StructureMasks& m, int32_t* out, hipStream_t st);

}  // namespace irlosc
