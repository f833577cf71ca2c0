"""``ActionSequenceRunner``: the WP / GRIP action-sequence state machine of the reference's insertion demo
(/root/reference/irl_control/examples/insertion_task.py:105-318, action list and action objects in
action_sequence_configs/insertion_task.yaml:35-103), headless and with the simulator injected.

Per tick it is the same hot path as every other caller — ``controller.generate(targets)``, forces into ``sim.data.ctrl``,
``sim.step()`` — around which the demo adds:
  * WP   go to a waypoint: the target is a list, 'start_pos', or an ACTION OBJECT (its free-joint pose in the simulator
         plus a named offset; the orientation target composes the object's yaw with the default gripper orientation,
         insertion_task.py:249-262); the arm's ``max_vel[0]`` is re-set every tick from the current error,
         clip(kp * error, min_speed_xyz, max_speed_xyz) (insertion_task.py:291-295), until the error drops under max_error;
  * GRIP hold the targets and drive the gripper actuator for a duration (wall-clock seconds in the reference,
         insertion_task.py:193-205; ``gripper_duration / tick_seconds`` ticks here, so that a run is reproducible).
``controller`` may be this package's OSC (HIP path) or anything with generate / calc_error (the golden of
tests/golden/loop_insertion_wp.npz was minted by the reference's own InsertionTask methods on the same FakeSim).
"""
import copy
import os
from enum import Enum
from typing import Dict, List, Optional

import numpy as np
import yaml

from .device import DeviceState
from .targets import Target
from .transforms import compose, euler2mat, euler2quat, mat2euler, quat2mat

_PKG_DIR = os.path.dirname(os.path.abspath(__file__))
DEFAULT_EE_ROT = np.deg2rad([0, -90, -90])                       # insertion_task.py:18
DEFAULT_EE_QUAT = euler2quat(*DEFAULT_EE_ROT)                    # insertion_task.py:20
GRIPPER_CTRL_IDX = {"ur5right": 7, "ur5left": 14}                # insertion_task.py:152-155


class Action(Enum):
    WP = 0
    GRIP = 1


DEFAULT_PARAMS = {                                               # insertion_task.py:83-103
    Action.WP: dict(kp=6, max_error=0.0018, gripper_force=0.0, min_speed_xyz=0.1, max_speed_xyz=3.0),
    Action.GRIP: dict(gripper_force=-0.08, gripper_duration=1.0),
}


def load_action_config(config_file: str = "insertion_task.yaml") -> Dict:
    path = config_file if os.path.isabs(config_file) else os.path.join(_PKG_DIR, "action_sequence_configs", config_file)
    with open(path) as f:
        return yaml.safe_load(f)


class ActionSequenceRunner:
    def __init__(self, app, controller, active_arm: str = "right", tick_seconds: float = 0.001, max_ticks_per_action: int = 20000,
                 on_tick=None):
        self.app, self.sim, self.controller = app, app.sim, controller
        self.robot = app.get_robot("DualUR5")
        self.ur5right, self.ur5left = self.robot.get_device("ur5right"), self.robot.get_device("ur5left")
        self.set_active_arm(active_arm)
        self.errors: Dict[str, float] = {}
        self.targets = {self.active_arm.name: Target(), self.passive_arm.name: Target()}
        self.action_objects: Dict = {}
        self.start_pos = None
        self.tick_seconds = tick_seconds
        self.max_ticks_per_action = max_ticks_per_action
        self.on_tick = on_tick                 # callback(runner, ctrlr_output) after every simulator step
        self.ticks = 0

    # ---- configuration ----------------------------------------------------------------------------------------------
    def set_active_arm(self, active_arm: str):
        assert active_arm in ("right", "left"), "Demo only supports Dual UR5 configuration"
        self.active_arm, self.passive_arm = (self.ur5right, self.ur5left) if active_arm == "right" else (self.ur5left, self.ur5right)

    def initialize_action_objects(self):
        """Place the action objects (their free joints) as the action-object table says (insertion_task.py:299-311)."""
        for obj in self.action_objects.values():
            quat = euler2quat(*np.deg2rad(obj["initial_pos_abg"])) if "initial_pos_abg" in obj else None
            self.app.set_free_joint_qpos(obj["joint_name"], quat=quat, pos=obj.get("initial_pos_xyz"))

    # ---- per-tick plumbing -------------------------------------------------------------------------------------------
    def send_forces(self, forces, gripper_force: Optional[float] = None, update_errors=None):
        for force_idx, force in zip(*forces):
            self.sim.data.ctrl[force_idx] = force
        if gripper_force:
            self.sim.data.ctrl[GRIPPER_CTRL_IDX[self.active_arm.name]] = gripper_force
        self.sim.step()
        self.ticks += 1
        names = [update_errors] if isinstance(update_errors, str) else (update_errors or [])
        for name in names:
            self.errors[name] = float(np.linalg.norm(self.controller.calc_error(self.targets[name], self.robot.get_device(name))))
        if self.on_tick is not None:
            self.on_tick(self, forces)

    # ---- actions ---------------------------------------------------------------------------------------------------------
    def set_waypoint_targets(self, params: Dict):
        self.targets[self.passive_arm.name].set_xyz(self.passive_arm.get_state(DeviceState.EE_XYZ))
        self.targets[self.passive_arm.name].set_quat(DEFAULT_EE_QUAT)
        if "target_xyz" not in params:
            raise KeyError("target_xyz")
        offset = params.get("offset", [0.0, 0.0, 0.0])
        txyz = params["target_xyz"]
        if isinstance(txyz, str):
            if txyz == "start_pos":
                target = self.start_pos
            else:
                obj = self.action_objects[txyz]
                if isinstance(offset, str):
                    offset = obj[offset]
                target = self.sim.data.get_joint_qpos(obj["joint_name"])[:3] + offset
        elif isinstance(txyz, list):
            target = txyz + offset                                   # list concatenation, as in the reference (:240)
        else:
            raise ValueError("Invalid type for target_xyz!")
        self.targets[self.active_arm.name].set_xyz(target)
        if "target_abg" in params:
            tabg = params["target_abg"]
            if isinstance(tabg, str):
                obj = self.action_objects[tabg]
                obj_quat = self.sim.data.get_joint_qpos(obj["joint_name"])[-4:]
                grip_eul = DEFAULT_EE_ROT + [0, 0, np.deg2rad(obj["grip_yaw"])]
                tfmat = np.matmul(compose([0, 0, 0], quat2mat(obj_quat), [1, 1, 1]),
                                  compose([0, 0, 0], euler2mat(*grip_eul), [1, 1, 1]))
                target_abg = np.array(mat2euler(tfmat[:3, :3]))
            elif isinstance(tabg, list):
                target_abg = np.deg2rad(tabg)
            else:
                raise ValueError("Invalid type for target_abg!")
            self.targets[self.active_arm.name].set_abg(target_abg)
        else:
            self.targets[self.active_arm.name].set_quat(DEFAULT_EE_QUAT)

    @staticmethod
    def _with_defaults(params: Dict, action: Action) -> Dict:
        for key, val in DEFAULT_PARAMS[action].items():
            params.setdefault(key, val)
        return params

    def go_to_waypoint(self, params: Dict):
        assert params["action"] == "WP"
        self.set_waypoint_targets(params)
        self._with_defaults(params, Action.WP)
        arm = self.active_arm.name
        self.errors[arm] = np.inf
        n = 0
        while self.errors[arm] > params["max_error"]:
            # error-adaptive velocity limit of the active arm (insertion_task.py:293-295)
            self.active_arm.max_vel[0] = max(params["min_speed_xyz"], min(params["max_speed_xyz"], params["kp"] * self.errors[arm]))
            self.send_forces(self.controller.generate(self.targets), gripper_force=params["gripper_force"], update_errors=arm)
            n += 1
            if n >= self.max_ticks_per_action:
                raise RuntimeError(f"waypoint not reached within {n} ticks (error {self.errors[arm]:.4g})")

    def grip(self, params: Dict):
        assert params["action"] == "GRIP"
        self._with_defaults(params, Action.GRIP)
        for _ in range(max(1, int(round(params["gripper_duration"] / self.tick_seconds)))):
            self.send_forces(self.controller.generate(self.targets), gripper_force=params["gripper_force"],
                             update_errors=self.active_arm.name)

    def run_sequence(self, action_sequence: List[Dict]):
        self.start_pos = np.copy(self.active_arm.get_state(DeviceState.EE_XYZ))
        for entry in action_sequence:
            entry = copy.deepcopy(entry)
            {"WP": self.go_to_waypoint, "GRIP": self.grip}[entry["action"]](entry)


# ---- the same state machine for a fleet: B robots, B independent object placements, one GPU step per tick --------------
def _calc_error_batch(ee_pose, tgt_pose):
    """OSC.calc_error (osc.py:101-118) for B poses: [xyz error, sxyz Euler angles of q_ee * conj(normalised q_tgt)]."""
    from .transforms import normalized_vector, qconjugate, qmult, quat2euler
    e = np.zeros((len(ee_pose), 6))
    e[:, :3] = ee_pose[:, :3] - tgt_pose[:, :3]
    for b in range(len(ee_pose)):
        q_r = np.array(qmult(normalized_vector(tgt_pose[b, 3:]), qconjugate(ee_pose[b, 3:])))
        e[b, 3:] = quat2euler(qconjugate(q_r))
    return e


def waypoint_target(obj, params, start_xyz):
    """Target pose (x y z qw qx qy qz) of a WP action for one robot: `obj` its action objects ({name: {"pos", "quat", offsets,
    "grip_yaw"}}), `start_xyz` the active arm's EE position at the start of the list ('start_pos').  The rule of
    insertion_task.py:228-262 on object poses that are given instead of read from a simulator."""
    offset = params.get("offset", [0.0, 0.0, 0.0])
    txyz = params["target_xyz"]
    if isinstance(txyz, str):
        if txyz == "start_pos":
            xyz = start_xyz
        else:
            o = obj[txyz]
            xyz = np.asarray(o["pos"]) + np.asarray(o[offset] if isinstance(offset, str) else offset)
    else:
        xyz = np.asarray(txyz, dtype=np.float64) + np.asarray(offset, dtype=np.float64)
    if "target_abg" in params:
        tabg = params["target_abg"]
        if isinstance(tabg, str):
            o = obj[tabg]
            grip_eul = DEFAULT_EE_ROT + [0, 0, np.deg2rad(o["grip_yaw"])]
            R = quat2mat(o["quat"]) @ euler2mat(*grip_eul)
            quat = euler2quat(*mat2euler(R))
        else:
            quat = euler2quat(*np.deg2rad(tabg))
    elif "target_quat" in params:                                    # the iros2022 dialect (action_motion.compile_iros2022): taken as given
        quat = np.asarray(params["target_quat"], dtype=np.float64)
    else:
        quat = DEFAULT_EE_QUAT
    return np.concatenate([xyz, quat])


class FleetActionSequenceRunner:
    """B robots run the SAME WP / GRIP action list, each on its own action objects (randomised poses), in lockstep on the
    batched controller: per tick one `BatchedOSC` step from joint coordinates (rigid-body front end on the GPU) with
    PER-INSTANCE gains, because the error-adaptive velocity limit of insertion_task.py:293-295 differs per robot.
    An instance that has finished its list holds its last targets.  The physics is whatever `integrate(q, qd, u, rec)`
    does (examples/insertion_fleet_headless.py: M qacc = u - bias with M, bias read back from HBM).

    Semantics per instance are those of ActionSequenceRunner (and the kernels make an instance's result independent of
    its batch-mates), so robot b of a fleet follows, bit for bit, the trajectory it follows alone
    (tests/test_gpu_parity.py::test_fleet_action_sequence_lockstep_equals_solo_runs)."""

    def __init__(self, osc, base_gains: Dict, objects: List[Dict], sequence: List[Dict], active_arm: str = "right",
                 tick_seconds: float = 0.001, passive_hold_orientation: bool = False, integrator_records=()):
        self.osc, self.lay = osc, osc.layout
        # records tick() hands back besides the EE poses it needs itself: a host-side integrator names what IT reads (e.g.
        # ("M", "bias")); by default only the 168 B of EE poses per robot cross PCIe per tick, not the 8.5 KB of records
        self.records = ("ee_pose",) + tuple(k for k in integrator_records if k != "ee_pose")
        # the reference sends the passive arm to DEFAULT_EE_QUAT at every waypoint (insertion_task.py:213), which suits the
        # start pose of its scene; with arbitrary start poses holding the current orientation keeps that arm where it is
        self.passive_hold_orientation = passive_hold_orientation
        self.B = len(objects)
        self.objects = objects                      # per instance: {name: {"pos": xyz, "quat": wxyz, **offsets, "grip_yaw"}}
        self.seq = [copy.deepcopy(e) for e in sequence]
        for e in self.seq:
            ActionSequenceRunner._with_defaults(e, Action.WP if e["action"] == "WP" else Action.GRIP)
        self.arm = "ur5right" if active_arm == "right" else "ur5left"
        self.other = "ur5left" if active_arm == "right" else "ur5right"
        self.ia, self.io = self.lay.dev_names.index(self.arm), self.lay.dev_names.index(self.other)
        self.base_gains = base_gains
        self.tick_seconds = tick_seconds
        self.action = np.zeros(self.B, dtype=int)                 # index of the action each instance is in
        self.grip_left = np.zeros(self.B, dtype=int)              # ticks left in a GRIP action
        self.err = np.full(self.B, np.inf)
        self.max_vel0 = np.zeros(self.B)
        self.gripper_force = np.zeros(self.B)
        self.tgt = None
        self.start_pos = None
        self.entered = np.full(self.B, -1)                        # action whose targets are currently set
        self.ticks = 0

    def _waypoint_target(self, b, params, ee_pose_b):
        return waypoint_target(self.objects[b], params, self.start_pos[b])

    def done(self):
        return self.action >= len(self.seq)

    def tick(self, q, qd):
        """One control tick for the fleet: returns (u[B,n], records) for the integrator (records: `integrator_records`)."""
        osc = self.osc
        osc.upload_q(q, qd)
        osc.frontend()
        rec = osc.download_records(keys=self.records)
        ee = rec["ee_pose"].astype(np.float64)
        if self.tgt is None:
            self.tgt = ee.copy()
            self.start_pos = ee[:, self.ia, :3].copy()
        for b in range(self.B):
            a = self.action[b]
            if a >= len(self.seq) or self.entered[b] == a:
                continue
            p = self.seq[a]
            self.entered[b] = a
            self.gripper_force[b] = p["gripper_force"]
            if p["action"] == "WP":
                self.tgt[b, self.io, :3] = ee[b, self.io, :3]            # passive arm holds position (insertion_task.py:212-213)
                self.tgt[b, self.io, 3:] = ee[b, self.io, 3:] if self.passive_hold_orientation else DEFAULT_EE_QUAT
                self.tgt[b, self.ia] = self._waypoint_target(b, p, ee[b])
                self.err[b] = np.inf
            else:
                self.grip_left[b] = max(1, int(round(p["gripper_duration"] / self.tick_seconds)))
        # error-adaptive velocity limit of the active arm, per instance
        mv = np.broadcast_to(np.asarray(self.base_gains["max_vel"], dtype=np.float64), (self.B, self.lay.ndev, 2)).copy()
        for b in range(self.B):
            a = self.action[b]
            if a < len(self.seq) and self.seq[a]["action"] == "WP":
                p = self.seq[a]
                self.max_vel0[b] = max(p["min_speed_xyz"], min(p["max_speed_xyz"], p["kp"] * self.err[b]))
            mv[b, self.ia, 0] = self.max_vel0[b] if self.max_vel0[b] > 0 else mv[b, self.ia, 0]
        g = self.base_gains
        osc.set_gains(g["kp"], g["kv"], g["ko"], g["k"], g["d"], mv, np.full(self.B, g["null_kv"]) if np.ndim(g["null_kv"]) == 0 else g["null_kv"])
        osc.set_targets(self.tgt)
        u = osc.step()
        self.ticks += 1
        return u, rec

    def after_step(self, ee_pose):
        """Bookkeeping after the simulator step (errors are measured on the new state, as in send_forces)."""
        e = np.linalg.norm(_calc_error_batch(ee_pose[:, self.ia], self.tgt[:, self.ia]), axis=1)
        for b in range(self.B):
            a = self.action[b]
            if a >= len(self.seq):
                continue
            self.err[b] = e[b]
            if self.seq[a]["action"] == "WP":
                if self.err[b] <= self.seq[a]["max_error"]:
                    self.action[b] += 1
            else:
                self.grip_left[b] -= 1
                if self.grip_left[b] <= 0:
                    self.action[b] += 1


# ---- the same list as data: what BatchedOSC.set_action_list hands to the GPU (include/irlosc.h, csrc/osc_action.hpp) -----------
def compile_action_list(sequence: List[Dict], objects: List[Dict], active_dev: int, passive_dev: int = -1, tick_seconds: float = 0.001,
                        passive_hold_orientation: bool = False, passive_quat=None) -> Dict:
    """The WP / GRIP list of FleetActionSequenceRunner as arrays: defaults from DEFAULT_PARAMS, per robot the pose table of its WP
    actions (waypoint_target on its action objects; 'start_pos' becomes the flag xyz_from_start, its xyz is taken on tick 0), and
    grip_ticks = max(1, round(gripper_duration / tick_seconds)).  -> the `desc` of action_list_tick / set_action_list."""
    seq = [ActionSequenceRunner._with_defaults(copy.deepcopy(e), Action.WP if e["action"] == "WP" else Action.GRIP) for e in sequence]
    A, B = len(seq), len(objects)
    d = dict(n_actions=A, active_dev=int(active_dev), passive_dev=int(passive_dev), passive_hold_orientation=int(bool(passive_hold_orientation)),
             passive_quat=np.asarray(DEFAULT_EE_QUAT if passive_quat is None else passive_quat, dtype=np.float64),
             kind=np.zeros(A, np.int32), xyz_from_start=np.zeros(A, np.int32), grip_ticks=np.ones(A, np.int32),
             kp=np.zeros(A), max_error=np.zeros(A), min_speed=np.zeros(A), max_speed=np.zeros(A), gripper_force=np.zeros(A),
             pose=np.zeros((B, A, 7)))
    d["pose"][:, :, 3] = 1.0                                          # (rows of GRIP actions are not read)
    for a, p in enumerate(seq):
        d["gripper_force"][a] = p["gripper_force"]
        if p["action"] == "WP":
            d["kind"][a] = Action.WP.value
            d["xyz_from_start"][a] = int(isinstance(p["target_xyz"], str) and p["target_xyz"] == "start_pos")
            d["kp"][a], d["max_error"][a] = p["kp"], p["max_error"]
            d["min_speed"][a], d["max_speed"][a] = p["min_speed_xyz"], p["max_speed_xyz"]
            for b in range(B):
                d["pose"][b, a] = waypoint_target(objects[b], p, np.zeros(3))
        else:
            d["kind"][a] = Action.GRIP.value
            d["grip_ticks"][a] = max(1, int(round(p["gripper_duration"] / tick_seconds)))
    return d


OBJECT_INDEX = {"male_object": 0, "female_object": 1}            # the action objects of the `nist` and `grommet` sets, as object indices


def grip_quat(obj: Dict):
    """The grip rotation of an action object: the quaternion of euler2mat(DEFAULT_EE_ROT + [0, 0, grip_yaw]) (insertion_task.py:252)."""
    return euler2quat(*(DEFAULT_EE_ROT + [0, 0, np.deg2rad(obj["grip_yaw"])]))


def compile_action_list_refs(sequence: List[Dict], objects: List[Dict], active_dev: int, passive_dev: int = -1, tick_seconds: float = 0.001,
                             passive_hold_orientation: bool = False, passive_quat=None):
    """compile_action_list for a slot with ACTION OBJECTS (BatchedOSC.set_objects): a WP that names an object aims at the object's pose
    AT THE MOMENT THE WP IS ENTERED, as set_waypoint_targets reads it from the simulator (insertion_task.py:226-262), not at the pose it
    had when the list was compiled.  -> (desc, refs, pose0):
      desc   compile_action_list's dict, but for a WP whose target_xyz names an object the xyz words of `pose` are the OFFSET (the
             named one of the object, or the list given), and for a WP whose target_abg names an object the quaternion words are the
             object's grip rotation (grip_quat)
      refs   dict(xyz_obj, quat_obj: int32 [A]): per action the object index (OBJECT_INDEX) or -1 -- BatchedOSC.set_action_refs
      pose0  [B, 2, 7] the objects' start poses (x y z qw qx qy qz) from each robot's {"pos", "quat"} -- BatchedOSC.set_objects
    With the objects at rest the targets the GPU composes -- object xyz + offset, q_obj (x) q_grip -- are compile_action_list's static
    table: the xyz words bit for bit, the quaternion to rounding and up to its sign (objects.ref_target; tests/test_objects_host.py)."""
    d = compile_action_list(sequence, objects, active_dev, passive_dev, tick_seconds, passive_hold_orientation, passive_quat)
    A, B = d["n_actions"], len(objects)
    refs = dict(xyz_obj=np.full(A, -1, np.int32), quat_obj=np.full(A, -1, np.int32))
    for a, p in enumerate(sequence):
        if p["action"] != "WP":
            continue
        txyz, tabg = p["target_xyz"], p.get("target_abg")
        if isinstance(txyz, str) and txyz != "start_pos":
            refs["xyz_obj"][a] = OBJECT_INDEX[txyz]
            offset = p.get("offset", [0.0, 0.0, 0.0])
            for b in range(B):
                d["pose"][b, a, :3] = np.asarray(objects[b][txyz][offset] if isinstance(offset, str) else offset, dtype=np.float64)
        if isinstance(tabg, str):
            refs["quat_obj"][a] = OBJECT_INDEX[tabg]
            for b in range(B):
                d["pose"][b, a, 3:] = grip_quat(objects[b][tabg])
    names = sorted(OBJECT_INDEX, key=OBJECT_INDEX.get)
    pose0 = np.array([[np.concatenate([np.asarray(o[nm]["pos"], dtype=np.float64), np.asarray(o[nm]["quat"], dtype=np.float64)]) for nm in names]
                      for o in objects])
    return d, refs, pose0


def action_list_state(B: int) -> Dict:
    """The per-robot state of an action list as irlosc_set_action_list resets it."""
    return dict(action=np.zeros(B, np.int32), entered=np.full(B, -1, np.int32), grip_left=np.zeros(B, np.int32),
                err=np.full(B, np.inf), max_vel0=np.zeros(B), gripper_force=np.zeros(B), finished_tick=np.full(B, -1, np.int32),
                start_xyz=np.zeros((B, 3)))


def action_list_tick(state: Dict, ee, tgt, gains, desc: Dict, t: int):
    """One tick of the action-list kernel (csrc/osc_action.hpp) in NumPy, in place: its four steps on rollout tick `t` of the list,
    i.e. FleetActionSequenceRunner.after_step of the PREVIOUS tick (judged on `ee`, the EE poses of the state that tick's step
    produced) followed by the bookkeeping of FleetActionSequenceRunner.tick.  A robot's list starts on the first tick that runs it
    (entered < 0: tick 0, or a later one when `ee` held fewer robots before): it is not judged then, its start_xyz is taken and action 0
    is entered; finished_tick is `t`, the slot's count, all the same.
      state  action_list_state(B), advanced in place
      ee     [B, ndev, 7] EE poses at the start of tick t
      tgt    [B, ndev, 7] targets as stored (any float dtype; entered WP actions write it, values rounded to its dtype)
      gains  [B, ndev, GAIN_WORDS] gain records as stored, or None: word 9 (max_vel0) of the active device is written
      desc   compile_action_list(...)"""
    A, ia, io = desc["n_actions"], desc["active_dev"], desc["passive_dev"]
    ee = np.asarray(ee, dtype=np.float64)
    B = len(ee)
    st = state
    first = st["entered"][:B] < 0
    if not first.all():
        live = (st["action"][:B] < A) & ~first
        e = np.linalg.norm(_calc_error_batch(ee[:, ia], np.asarray(tgt[:B, ia], dtype=np.float64)), axis=1)
        for b in np.nonzero(live)[0]:
            a = st["action"][b]
            st["err"][b] = e[b]
            if desc["kind"][a] == Action.WP.value:
                nxt = st["err"][b] <= desc["max_error"][a]
            else:
                st["grip_left"][b] -= 1
                nxt = st["grip_left"][b] <= 0
            if nxt:
                st["action"][b] += 1
                if st["action"][b] == A:
                    st["finished_tick"][b] = t
    st["start_xyz"][:B][first] = ee[first, ia, :3]
    pose = desc["pose"]
    for b in range(B):
        a = st["action"][b]
        if a >= A:
            continue
        if st["entered"][b] != a:
            st["entered"][b] = a
            st["gripper_force"][b] = desc["gripper_force"][a]
            if desc["kind"][a] == Action.WP.value:
                if io >= 0:
                    tgt[b, io, :3] = ee[b, io, :3]
                    tgt[b, io, 3:] = ee[b, io, 3:] if desc["passive_hold_orientation"] else desc["passive_quat"]
                tgt[b, ia] = pose[b if len(pose) > 1 else 0, a]
                if desc["xyz_from_start"][a]:
                    tgt[b, ia, :3] = st["start_xyz"][b]
                st["err"][b] = np.inf
            else:
                st["grip_left"][b] = desc["grip_ticks"][a]
        if desc["kind"][a] == Action.WP.value:
            with np.errstate(invalid="ignore"):      # (kp 0 on the tick a WP is entered: 0 x inf = NaN, which min() passes over like the kernel)
                st["max_vel0"][b] = max(desc["min_speed"][a], min(desc["max_speed"][a], desc["kp"][a] * st["err"][b]))
            if gains is not None:
                gains[b, ia, 9] = st["max_vel0"][b]
    return state
