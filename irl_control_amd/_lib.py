"""ctypes binding of libirlosc.so (include/irlosc.h).  Loads the in-tree library; there is no
fallback: if the HIP library is missing or no GPU is present, compute calls raise."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("IRLOSC_LIB", os.path.join(_HERE, "libirlosc.so"))   # override: A/B builds only

MAX_DEV, MAX_N, MAX_K, GAIN_WORDS, MAX_BODIES = 4, 32, 16, 12, 64
MAX_WAYPOINTS = 64
MAX_ACTIONS = 32
MAX_PUSHES = 8
MAX_WALLS = 8
MAX_JOINT_ROWS = 48
JOINT_LIMIT, JOINT_COUPLE, JOINT_DRIVE = 0, 1, 2
JOINT_SRC_CONST, JOINT_SRC_ACTION = 0, 1
ACTION_WP, ACTION_GRIP = 0, 1
MAX_STREAM_TICKS = 16384
TELEOP_NONE, TELEOP_RIGID, TELEOP_HEADING = 0, 1, 2
POLICY_MAX_IN, POLICY_MAX_WIDTH, POLICY_MAX_LAYERS = 192, 128, 4
OBS_QPOS, OBS_QVEL, OBS_EE_POSE, OBS_TARGETS, OBS_WRENCH, OBS_PLATE, OBS_OBJECT_POSE = (1 << i for i in range(7))
F32, F64 = 0, 1
USE_G, ADMITTANCE, NULLSPACE = 1, 2, 4
KERNEL_AUTO, KERNEL_GENERIC, KERNEL_ROW16 = 0, 1, 3      # (2: the fp32-arithmetic kernel removed in ABI version 3)
FLAG_M_NOT_PD, FLAG_PINV_BRANCH, FLAG_EIGEN_PATH, FLAG_TRUNCATED = 1, 2, 4, 8
FLAG_VEL_BRANCH_B, FLAG_BAD_JIDX, FLAG_NONFINITE = 16, 32, 64

EXPORTS = ["irlosc_abi_version", "irlosc_device_count", "irlosc_create", "irlosc_destroy",
           "irlosc_last_error", "irlosc_kernel_name", "irlosc_frontend_name", "irlosc_set_gains", "irlosc_upload",
           "irlosc_set_targets", "irlosc_step", "irlosc_step_resident", "irlosc_download",
           "irlosc_sync", "irlosc_step_device", "irlosc_time_dominant_kernel",
           "irlosc_steps_per_launch", "irlosc_upload_raw", "irlosc_upload_raw_sparse", "irlosc_assemble_device", "irlosc_device_sync",
           "irlosc_tick", "irlosc_comm_unique_id", "irlosc_comm_create", "irlosc_comm_destroy",
           "irlosc_comm_last_error", "irlosc_bench_allreduce", "irlosc_comm_allgather_u64", "irlosc_set_model",
           "irlosc_upload_q", "irlosc_frontend", "irlosc_step_resident_from_q", "irlosc_download_records",
           "irlosc_step_from_q", "irlosc_from_q_name", "irlosc_slot_structure", "irlosc_probe_structure", "irlosc_time_trains", "irlosc_giveup_counts",
           "irlosc_kernel_class", "irlosc_set_ft_sensors", "irlosc_set_sensordata", "irlosc_step_from_q_device",
           "irlosc_slot_route", "irlosc_set_plant", "irlosc_rollout_from_q", "irlosc_download_q",
           "irlosc_set_waypoints", "irlosc_download_waypoint_state", "irlosc_set_action_list", "irlosc_download_action_state",
           "irlosc_set_pushes", "irlosc_set_walls", "irlosc_download_wall_state", "irlosc_set_joints",
           "irlosc_download_joint_state", "irlosc_set_teleop_stream", "irlosc_download_teleop_state", "irlosc_download_targets",
           "irlosc_log_layout", "irlosc_rollout_from_q_logged", "irlosc_set_episodes", "irlosc_download_episode_state",
           "irlosc_set_objects", "irlosc_download_object_state", "irlosc_set_action_refs", "irlosc_log_layout_objects",
           "irlosc_set_action_motion", "irlosc_download_action_motion_state", "irlosc_set_object_loads",
           "irlosc_download_object_load_state", "irlosc_set_policy", "irlosc_download_policy_state",
           "irlosc_set_policy_noise", "irlosc_download_policy_noise_state", "irlosc_log_layout_policy",
           "irlosc_set_reward", "irlosc_download_reward_state", "irlosc_log_layout_reward"]
LOG_QPOS, LOG_QVEL, LOG_EE_POSE, LOG_TARGETS, LOG_WRENCH, LOG_U, LOG_FLAGS, LOG_WALL_FORCE, LOG_JOINT_TAU = (1 << i for i in range(9))
LOG_OBJECT_POSE = 512                                    # only on a slot with action objects
LOG_POLICY_OUT, LOG_POLICY_SAMPLE = 1024, 2048           # only on a slot with a policy / one whose policy has a Gaussian head
LOG_REWARD = 4096                                        # only on a slot with a reward
EPISODE_FINISHED, EPISODE_TIMEOUT, EPISODE_INSERTED, EPISODE_GOAL = 1, 2, 4, 8
MAX_REWARD_TERMS, MAX_REWARD_POINTS = 8, 8
REWARD_EE, REWARD_TARGET, REWARD_OBJECT, REWARD_FIXED = 0, 1, 2, 3      # point kinds
REWARD_DIST_SQ, REWARD_DIST, REWARD_ORI, REWARD_ACT_SQ, REWARD_U_SQ, REWARD_FORCE, REWARD_MATED, REWARD_ONE = range(8)      # term kinds
MAX_OBJECTS, MAX_GRIPPERS, MAX_MATES = 4, 2, 2
MAX_EPISODE_RECORDS, MAX_EPISODE_STARTS = 16, 4096
ABI_VERSION = 3
CLASS_GENERIC, CLASS_ROW16, CLASS_ROW16_PADDED = 0, 1, 2
ROUTE_NONE, ROUTE_GENERIC, ROUTE_ROW16, ROUTE_ROW16_TREE, ROUTE_LANE = 0, 1, 2, 3, 4
COMM_ID_BYTES = 128


class RawDesc(C.Structure):
    """struct irlosc_raw_desc (include/irlosc.h)."""
    _fields_ = [("nv", C.c_int32), ("n_sensor", C.c_int32), ("joint_ids", C.c_int32 * 32),
                ("dq_src", C.c_int32 * 32), ("ft_force0", C.c_int32 * 4), ("ft_torque0", C.c_int32 * 4)]


MAX_NV = 128


class QmLayout(C.Structure):
    """struct irlosc_qm_layout (include/irlosc.h): MuJoCo's sparse form of M -- mjModel.nM, dof_Madr, dof_parentid."""
    _fields_ = [("nM", C.c_int32), ("dof_Madr", C.c_int32 * MAX_NV), ("dof_parentid", C.c_int32 * MAX_NV)]


class Model(C.Structure):
    """struct irlosc_model (include/irlosc.h)."""
    _fields_ = [("nb", C.c_int32), ("nj", C.c_int32), ("parent", C.c_int32 * MAX_BODIES),
                ("joint_of_body", C.c_int32 * MAX_BODIES), ("pos", (C.c_double * 3) * MAX_BODIES),
                ("quat", (C.c_double * 4) * MAX_BODIES), ("jaxis", (C.c_double * 3) * MAX_N),
                ("jpos", (C.c_double * 3) * MAX_N), ("armature", C.c_double * MAX_N), ("mass", C.c_double * MAX_BODIES),
                ("ipos", (C.c_double * 3) * MAX_BODIES), ("iquat", (C.c_double * 4) * MAX_BODIES),
                ("inertia", (C.c_double * 3) * MAX_BODIES), ("gravity", C.c_double * 3), ("ee_body", C.c_int32 * MAX_DEV)]


class FtDesc(C.Structure):
    """struct irlosc_ft_desc (include/irlosc.h): the F/T site of each target device (body, frame in it) and its sensordata slices."""
    _fields_ = [("n_sensor", C.c_int32), ("site_body", C.c_int32 * MAX_DEV), ("site_quat", (C.c_double * 4) * MAX_DEV),
                ("ft_force0", C.c_int32 * MAX_DEV), ("ft_torque0", C.c_int32 * MAX_DEV)]


class Plant(C.Structure):
    """struct irlosc_plant (include/irlosc.h): the contact-free plant of irlosc_rollout_from_q."""
    _fields_ = [("dt", C.c_double), ("damping", C.c_double), ("ctrl_mask", C.c_uint32), ("reserved", C.c_uint32)]


class Waypoints(C.Structure):
    """struct irlosc_waypoints (include/irlosc.h): the waypoint paths of irlosc_set_waypoints."""
    _fields_ = [("count", C.c_int32 * MAX_DEV), ("threshold", C.c_double * MAX_DEV), ("loop", C.c_uint8 * MAX_DEV), ("nb", C.c_int32)]


class ActionList(C.Structure):
    """struct irlosc_action_list (include/irlosc.h): the WP / GRIP action list of irlosc_set_action_list."""
    _fields_ = [("n_actions", C.c_int32), ("active_dev", C.c_int32), ("passive_dev", C.c_int32), ("passive_hold_orientation", C.c_int32),
                ("passive_quat", C.c_double * 4), ("nb", C.c_int32),
                ("kind", C.c_int32 * MAX_ACTIONS), ("xyz_from_start", C.c_int32 * MAX_ACTIONS), ("grip_ticks", C.c_int32 * MAX_ACTIONS),
                ("kp", C.c_double * MAX_ACTIONS), ("max_error", C.c_double * MAX_ACTIONS), ("min_speed", C.c_double * MAX_ACTIONS),
                ("max_speed", C.c_double * MAX_ACTIONS), ("gripper_force", C.c_double * MAX_ACTIONS)]


class TeleopStream(C.Structure):
    """struct irlosc_teleop_stream (include/irlosc.h): the teleoperation stream of irlosc_set_teleop_stream."""
    _fields_ = [("ticks", C.c_int32), ("nb", C.c_int32), ("nb_origin", C.c_int32), ("loop", C.c_int32), ("increment", C.c_double),
                ("kind", C.c_int32 * MAX_DEV), ("off_xyz", (C.c_double * 3) * MAX_DEV), ("off_quat", (C.c_double * 4) * MAX_DEV),
                ("heading_offset", C.c_double * MAX_DEV)]


class Policy(C.Structure):
    """struct irlosc_policy (include/irlosc.h): the policy of irlosc_set_policy."""
    _fields_ = [("obs", C.c_uint32), ("n_layers", C.c_int32), ("width", C.c_int32 * POLICY_MAX_LAYERS), ("n_out", C.c_int32),
                ("keep_obs", C.c_int32), ("grip_dev", C.c_int32), ("nb_origin", C.c_int32), ("clip", C.c_float), ("reserved", C.c_int32),
                ("grip_close", C.c_double), ("grip_open", C.c_double), ("increment", C.c_double),
                ("kind", C.c_int32 * MAX_DEV), ("off_xyz", (C.c_double * 3) * MAX_DEV), ("off_quat", (C.c_double * 4) * MAX_DEV),
                ("heading_offset", C.c_double * MAX_DEV)]


class Pushes(C.Structure):
    """struct irlosc_pushes (include/irlosc.h): the external pushes of irlosc_set_pushes."""
    _fields_ = [("n_pushes", C.c_int32), ("nb", C.c_int32), ("dev", C.c_int32 * MAX_PUSHES), ("tick0", C.c_int32 * MAX_PUSHES),
                ("tick1", C.c_int32 * MAX_PUSHES), ("apply", C.c_uint8 * MAX_PUSHES), ("sense", C.c_uint8 * MAX_PUSHES)]


class Walls(C.Structure):
    """struct irlosc_walls (include/irlosc.h): the compliant walls of irlosc_set_walls."""
    _fields_ = [("n_walls", C.c_int32), ("nb", C.c_int32), ("dev", C.c_int32 * MAX_WALLS)]


class JointRows(C.Structure):
    """struct irlosc_joint_rows (include/irlosc.h): the joint rows of irlosc_set_joints."""
    _fields_ = [("n_rows", C.c_int32), ("per_robot", C.c_int32), ("kind", C.c_int32 * MAX_JOINT_ROWS),
                ("joint_a", C.c_int32 * MAX_JOINT_ROWS), ("joint_b", C.c_int32 * MAX_JOINT_ROWS),
                ("source", C.c_int32 * MAX_JOINT_ROWS), ("dev", C.c_int32 * MAX_JOINT_ROWS)]


class Log(C.Structure):
    """struct irlosc_log (include/irlosc.h): the episode log of irlosc_rollout_from_q_logged."""
    _fields_ = [("channels", C.c_uint32), ("every", C.c_int32), ("n_robots", C.c_int32), ("reserved", C.c_int32),
                ("buffer_bytes", C.c_uint64)]


class Episodes(C.Structure):
    """struct irlosc_episodes (include/irlosc.h): the episodes of irlosc_set_episodes."""
    _fields_ = [("max_ticks", C.c_int32), ("end_on_finish", C.c_int32), ("max_episodes", C.c_int32), ("n_starts", C.c_int32),
                ("starts_per_robot", C.c_int32), ("n_variants", C.c_int32), ("records", C.c_int32), ("poll_every", C.c_int32),
                ("reserved", C.c_int32)]


class Objects(C.Structure):
    """struct irlosc_objects (include/irlosc.h): the action objects of irlosc_set_objects."""
    _fields_ = [("n_objects", C.c_int32), ("n_grippers", C.c_int32), ("n_mates", C.c_int32), ("n_variants", C.c_int32),
                ("dev", C.c_int32 * MAX_GRIPPERS), ("joint", C.c_int32 * MAX_GRIPPERS), ("sign", C.c_int32 * MAX_GRIPPERS),
                ("plug", C.c_int32 * MAX_MATES), ("socket", C.c_int32 * MAX_MATES),
                ("q_close", C.c_double * MAX_GRIPPERS), ("q_open", C.c_double * MAX_GRIPPERS), ("grip_xyz", (C.c_double * 3) * MAX_GRIPPERS),
                ("radius", C.c_double * MAX_OBJECTS), ("seat_xyz", (C.c_double * 3) * MAX_MATES), ("seat_quat", (C.c_double * 4) * MAX_MATES),
                ("tol_xyz", C.c_double * MAX_MATES), ("min_abs_dot", C.c_double * MAX_MATES)]


class ObjectLoads(C.Structure):
    """struct irlosc_object_loads (include/irlosc.h): the weight of the slot's action objects, irlosc_set_object_loads."""
    _fields_ = [("per_robot", C.c_int32), ("reserved", C.c_int32), ("gravity", C.c_double * 3)]


class ActionRefs(C.Structure):
    """struct irlosc_action_refs (include/irlosc.h): the objects a list's WP actions aim at, irlosc_set_action_refs."""
    _fields_ = [("xyz_obj", C.c_int32 * MAX_ACTIONS), ("quat_obj", C.c_int32 * MAX_ACTIONS)]


class ActionMotion(C.Structure):
    """struct irlosc_action_motion (include/irlosc.h): INTERP steps and target noise of the list in force, irlosc_set_action_motion."""
    _fields_ = [("steps", C.c_int32 * MAX_ACTIONS), ("noise_mean", C.c_double * MAX_ACTIONS), ("noise_std", C.c_double * MAX_ACTIONS),
                ("seed", C.c_uint64)]


class PolicyNoise(C.Structure):
    """struct irlosc_policy_noise (include/irlosc.h): the Gaussian head of the policy in force, irlosc_set_policy_noise."""
    _fields_ = [("seed", C.c_uint64), ("n_std", C.c_int32), ("reserved", C.c_int32), ("std", C.c_float * 8)]


class Reward(C.Structure):
    """struct irlosc_reward (include/irlosc.h): the weighted terms, the discount and the goal of a slot's reward, irlosc_set_reward."""
    _fields_ = [("n_terms", C.c_int32), ("n_points", C.c_int32), ("points_per_robot", C.c_int32), ("goal_term", C.c_int32),
                ("goal_cmp", C.c_int32), ("goal_hold", C.c_int32), ("kind", C.c_int32 * 8), ("a_kind", C.c_int32 * 8),
                ("a_index", C.c_int32 * 8), ("b_kind", C.c_int32 * 8), ("b_index", C.c_int32 * 8), ("reserved", C.c_int32 * 2),
                ("weight", C.c_double * 8), ("gamma", C.c_double), ("goal_value", C.c_double)]


class Cfg(C.Structure):
    _fields_ = [("hip_device", C.c_int32), ("dtype", C.c_int32), ("max_batch", C.c_int32),
                ("n_slots", C.c_int32), ("n", C.c_int32), ("ndev", C.c_int32),
                ("flags", C.c_uint32), ("kernel", C.c_int32),
                ("dev_rows", C.c_int32 * MAX_DEV),
                ("ctrlr_dof", (C.c_uint8 * 6) * MAX_DEV),
                ("calc_xyz", C.c_uint8 * MAX_DEV), ("calc_abg", C.c_uint8 * MAX_DEV),
                ("joint_mask", C.c_uint32 * MAX_DEV), ("j_idx0", C.c_int32 * MAX_DEV)]


class IrloscError(RuntimeError):
    pass


_lib = None


def load():
    """Load libirlosc.so (built by __graft_entry__.build()).  Raises if absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise IrloscError(f"{LIB_PATH} not built: run `python __graft_entry__.py` "
                          "(hipcc --offload-arch=gfx950); there is no CPU fallback")
    lib = C.CDLL(LIB_PATH)
    vp, i32 = C.c_void_p, C.c_int32
    lib.irlosc_abi_version.restype = C.c_int
    if lib.irlosc_abi_version() != ABI_VERSION:
        raise IrloscError(f"{LIB_PATH} has ABI version {lib.irlosc_abi_version()}, this binding is written for {ABI_VERSION}: "
                          "rebuild with `python __graft_entry__.py`")
    lib.irlosc_device_count.restype = C.c_int
    lib.irlosc_create.argtypes = [C.POINTER(Cfg), C.POINTER(vp)]
    lib.irlosc_destroy.argtypes = [vp]
    lib.irlosc_destroy.restype = None
    lib.irlosc_last_error.argtypes = [vp]
    lib.irlosc_last_error.restype = C.c_char_p
    lib.irlosc_kernel_name.argtypes = [vp]
    lib.irlosc_kernel_name.restype = C.c_char_p
    lib.irlosc_kernel_class.argtypes = [vp]
    lib.irlosc_kernel_class.restype = C.c_int
    lib.irlosc_frontend_name.argtypes = [vp]
    lib.irlosc_frontend_name.restype = C.c_char_p
    lib.irlosc_set_gains.argtypes = [vp, vp, vp, i32]
    lib.irlosc_upload.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp, vp]
    lib.irlosc_set_targets.argtypes = [vp, i32, i32, vp, vp]
    lib.irlosc_step.argtypes = [vp, i32, i32, vp, vp]
    lib.irlosc_step_resident.argtypes = [vp, i32, i32, i32, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    lib.irlosc_time_dominant_kernel.argtypes = [vp, i32, i32, i32, C.POINTER(C.c_float)]
    lib.irlosc_steps_per_launch.argtypes = [vp]
    lib.irlosc_time_trains.argtypes = [vp, i32, i32, i32, i32, vp]
    lib.irlosc_giveup_counts.argtypes = [vp, vp]
    lib.irlosc_upload_raw.argtypes = [vp, i32, i32, C.POINTER(RawDesc)] + [vp] * 9
    lib.irlosc_upload_raw_sparse.argtypes = [vp, i32, i32, C.POINTER(RawDesc), C.POINTER(QmLayout)] + [vp] * 9
    lib.irlosc_assemble_device.argtypes = [vp, i32, i32, C.POINTER(RawDesc)] + [vp] * 10
    lib.irlosc_download.argtypes = [vp, i32, vp, vp]
    lib.irlosc_sync.argtypes = [vp]
    lib.irlosc_step_device.argtypes = [vp, i32] + [vp] * 11
    lib.irlosc_device_sync.argtypes = [vp]
    lib.irlosc_set_model.argtypes = [vp, C.POINTER(Model)]
    lib.irlosc_upload_q.argtypes = [vp, i32, i32, vp, vp]
    lib.irlosc_frontend.argtypes = [vp, i32, i32]
    lib.irlosc_download_records.argtypes = [vp, i32, i32] + [vp] * 5
    lib.irlosc_step_resident_from_q.argtypes = [vp, i32, i32, i32, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    lib.irlosc_step_from_q.argtypes = [vp, i32, i32, vp, vp]
    lib.irlosc_from_q_name.argtypes = [vp]
    lib.irlosc_set_ft_sensors.argtypes = [vp, C.POINTER(FtDesc)]
    lib.irlosc_set_sensordata.argtypes = [vp, i32, i32, vp]
    lib.irlosc_step_from_q_device.argtypes = [vp, i32, i32] + [vp] * 8
    lib.irlosc_from_q_name.restype = C.c_char_p
    lib.irlosc_set_plant.argtypes = [vp, C.POINTER(Plant)]
    lib.irlosc_rollout_from_q.argtypes = [vp, i32, i32, i32, i32, vp, vp, vp]
    lib.irlosc_download_q.argtypes = [vp, i32, i32, vp, vp]
    lib.irlosc_log_layout.argtypes = [i32, i32, C.c_uint32, i32, vp, vp]
    lib.irlosc_rollout_from_q_logged.argtypes = [vp, i32, i32, i32, C.POINTER(Log), vp, vp, vp, vp]
    lib.irlosc_set_waypoints.argtypes = [vp, i32, i32, C.POINTER(Waypoints), vp]
    lib.irlosc_download_waypoint_state.argtypes = [vp, i32, i32, vp, vp, vp]
    lib.irlosc_set_action_list.argtypes = [vp, i32, i32, C.POINTER(ActionList), vp]
    lib.irlosc_download_action_state.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp, vp]
    lib.irlosc_set_teleop_stream.argtypes = [vp, i32, i32, C.POINTER(TeleopStream), vp, vp]
    lib.irlosc_download_teleop_state.argtypes = [vp, i32, i32, vp, vp]
    lib.irlosc_download_targets.argtypes = [vp, i32, i32, vp]
    lib.irlosc_set_policy.argtypes = [vp, i32, i32, C.POINTER(Policy), vp, vp]
    lib.irlosc_download_policy_state.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp]
    lib.irlosc_set_policy_noise.argtypes = [vp, i32, C.POINTER(PolicyNoise), vp]
    lib.irlosc_download_policy_noise_state.argtypes = [vp, i32, i32, vp, vp, vp, vp]
    lib.irlosc_log_layout_policy.argtypes = [i32, i32, i32, i32, i32, C.c_uint32, i32, vp, vp]
    lib.irlosc_set_reward.argtypes = [vp, i32, i32, C.POINTER(Reward), vp]
    lib.irlosc_download_reward_state.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp, vp, vp]
    lib.irlosc_log_layout_reward.argtypes = [i32, i32, i32, i32, i32, i32, C.c_uint32, i32, vp, vp]
    lib.irlosc_set_pushes.argtypes = [vp, i32, i32, C.POINTER(Pushes), vp]
    lib.irlosc_set_walls.argtypes = [vp, i32, i32, C.POINTER(Walls), vp]
    lib.irlosc_download_wall_state.argtypes = [vp, i32, i32, vp, vp, vp, vp]
    lib.irlosc_set_joints.argtypes = [vp, i32, i32, C.POINTER(JointRows), vp]
    lib.irlosc_download_joint_state.argtypes = [vp, i32, i32, vp, vp, vp, vp]
    lib.irlosc_set_episodes.argtypes = [vp, i32, i32, C.POINTER(Episodes), vp, vp, vp]
    lib.irlosc_download_episode_state.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp, vp]
    lib.irlosc_set_objects.argtypes = [vp, i32, i32, C.POINTER(Objects), vp]
    lib.irlosc_download_object_state.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp, vp]
    lib.irlosc_set_object_loads.argtypes = [vp, i32, i32, C.POINTER(ObjectLoads), vp]
    lib.irlosc_download_object_load_state.argtypes = [vp, i32, i32, vp, vp]
    lib.irlosc_set_action_refs.argtypes = [vp, i32, C.POINTER(ActionRefs)]
    lib.irlosc_log_layout_objects.argtypes = [i32, i32, i32, C.c_uint32, i32, vp, vp]
    lib.irlosc_set_action_motion.argtypes = [vp, i32, C.POINTER(ActionMotion), vp]
    lib.irlosc_download_action_motion_state.argtypes = [vp, i32, i32, vp, vp, vp, vp]
    lib.irlosc_slot_structure.argtypes = [vp, C.c_int32]
    lib.irlosc_slot_structure.restype = C.c_int
    lib.irlosc_slot_route.argtypes = [vp, C.c_int32, C.c_int32]
    lib.irlosc_slot_route.restype = C.c_int
    lib.irlosc_probe_structure.argtypes = [vp, C.c_int32, C.c_int32]
    lib.irlosc_probe_structure.restype = C.c_int
    lib.irlosc_tick.argtypes = [vp, i32] + [vp] * 10
    lib.irlosc_comm_unique_id.argtypes = [vp]
    lib.irlosc_comm_create.argtypes = [i32, i32, i32, vp, C.POINTER(vp)]
    lib.irlosc_comm_destroy.argtypes = [vp]
    lib.irlosc_comm_destroy.restype = None
    lib.irlosc_comm_last_error.argtypes = [vp]
    lib.irlosc_comm_last_error.restype = C.c_char_p
    lib.irlosc_bench_allreduce.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    lib.irlosc_comm_allgather_u64.argtypes = [vp, C.c_uint64, vp]
    for name in EXPORTS:
        getattr(lib, name)
    _lib = lib
    return lib


def ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def np_dtype(dtype_code):
    return np.float64 if dtype_code == F64 else np.float32
