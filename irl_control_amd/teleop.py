"""The space-mouse teleoperation stream as data: what BatchedOSC.set_teleop_stream hands to the GPU (include/irlosc.h,
csrc/osc_teleop.hpp), and the NumPy mirror of the kernel's arithmetic.

The reference's demo (examples/space_mouse_example.py::run_demo, here examples/teleop_loops.py::space_mouse_loop) integrates the
device's rate readings into a plate pose (input_devices/space_mouse.py::SpaceMouse.update_state), lets both arms' targets ride on the
plate and turns the base towards it.  `stream_step` is one tick of that for one robot in the kernel's own operation order: every
product and sum on its own, written out, so that but for sin / cos / atan2 (libm here, the device's there) both sides round alike.

ps_move (examples/teleop_loops.py::ps_move_loop) has no resident form: its trigger switches ctrlr_dof_abg per tick, which changes the
number of task rows, and a context's layout is fixed when it is created.
"""
import math

import numpy as np

from . import _lib
from .transforms import euler2quat

NONE, RIGID, HEADING = _lib.TELEOP_NONE, _lib.TELEOP_RIGID, _lib.TELEOP_HEADING
INCREMENT = 0.0015                                   # input_devices/space_mouse.py: SpaceMouse's default step
ORIGIN = (0.0, 0.5, 0.5, 0.0, 0.0, 0.0)              # space_mouse_example.py:117


def follower(kind=NONE, off_xyz=(0.0, 0.0, 0.0), off_quat=(1.0, 0.0, 0.0, 0.0), heading_offset=0.0):
    """One device's entry of a rig: RIGID -- target pose = plate pose o (off_xyz, off_quat); HEADING -- target quaternion = the turn
    about world z by atan2(y, x) + heading_offset, xyz untouched; NONE -- the device keeps its target."""
    return dict(kind=int(kind), off_xyz=np.array(off_xyz, dtype=np.float64), off_quat=np.array(off_quat, dtype=np.float64),
                heading_offset=float(heading_offset))


def space_mouse_rig(layout):
    """The demo's followers for the devices of `layout` (teleop_loops.py:39-48), in its targets order: ur5right rides 0.2 m along the
    plate's x (0.05 + 0.15 in the reference's two transforms) with the plate's orientation, ur5left -0.2 m and turned by pi about the
    plate's z (mirrored grippers), the base faces the plate: atan2(y, x) - pi / 2.  Devices the layout lacks are dropped; others
    keep their targets."""
    demo = {"ur5right": follower(RIGID, (0.2, 0.0, 0.0)),
            "ur5left": follower(RIGID, (-0.2, 0.0, 0.0), euler2quat(0.0, 0.0, math.pi)),
            "base": follower(HEADING, heading_offset=-math.pi / 2)}
    return [demo.get(name, follower()) for name in layout.dev_names]


def _wrap(a):
    return float(np.arctan2(np.sin(a), np.cos(a)))      # SpaceMouse.constrain_angle, with its functions: the poses are bit-equal to it


def stream_step(pose, reading, rig, inc=INCREMENT):
    """One tick of one robot: pose (x y z roll pitch yaw) and the tick's reading (the same six, as rates) -> (new pose [6], targets
    [ndev, 7] with NaN in every word the tick does not write).  The kernel's arithmetic in the kernel's order (csrc/osc_teleop.hpp)."""
    x, y, z, roll, pitch, yaw = (float(v) for v in pose)
    r = [float(v) for v in reading]
    inc = float(inc)
    x = x + inc * r[0]
    y = y + inc * r[1]
    z = z + inc * r[2]
    yaw = _wrap(yaw - inc * r[5])
    pitch = _wrap(pitch - inc * r[4])
    roll = _wrap(roll + inc * r[3])
    # q_p = qx(pitch) (x) qy(roll) (x) qz(yaw): euler2quat(pitch, roll, yaw, axes='rxyz')
    hx, hy, hz = pitch * 0.5, roll * 0.5, yaw * 0.5
    cx, sx, cy, sy, cz, sz = math.cos(hx), math.sin(hx), math.cos(hy), math.sin(hy), math.cos(hz), math.sin(hz)
    cc, ss, sc, cs = cy * cz, sy * sz, sy * cz, cy * sz
    qw, qx, qy, qz = cx * cc - sx * ss, cx * ss + sx * cc, cx * sc - sx * cs, cx * cs + sx * sc
    # R(q_p): transforms.quat2mat
    Nq = qw * qw + qx * qx + qy * qy + qz * qz
    s = 2.0 / Nq
    X, Y, Z = qx * s, qy * s, qz * s
    wX, wY, wZ = qw * X, qw * Y, qw * Z
    xX, xY, xZ = qx * X, qx * Y, qx * Z
    yY, yZ, zZ = qy * Y, qy * Z, qz * Z
    R = ((1.0 - (yY + zZ), xY - wZ, xZ + wY), (xY + wZ, 1.0 - (xX + zZ), yZ - wX), (xZ - wY, yZ + wX, 1.0 - (xX + yY)))
    p = (x, y, z)
    tgt = np.full((len(rig), 7), np.nan)
    for d, f in enumerate(rig):
        if f["kind"] == RIGID:
            o = [float(v) for v in f["off_xyz"]]
            q0, q1, q2, q3 = (float(v) for v in f["off_quat"])
            for c in range(3):
                tgt[d, c] = p[c] + ((R[c][0] * o[0] + R[c][1] * o[1]) + R[c][2] * o[2])
            tgt[d, 3] = qw * q0 - qx * q1 - qy * q2 - qz * q3
            tgt[d, 4] = qw * q1 + qx * q0 + qy * q3 - qz * q2
            tgt[d, 5] = qw * q2 + qy * q0 + qz * q1 - qx * q3
            tgt[d, 6] = qw * q3 + qz * q0 + qx * q2 - qy * q1
        elif f["kind"] == HEADING:
            h = (math.atan2(y, x) + f["heading_offset"]) * 0.5
            tgt[d, 3:] = (math.cos(h), 0.0, 0.0, math.sin(h))
    return np.array([x, y, z, roll, pitch, yaw]), tgt


def stream_run(origin, readings, rig, inc=INCREMENT, targets=None):
    """T ticks of one robot: -> (poses [T, 6], targets [T, ndev, 7]); the words no tick writes are those of `targets` [ndev, 7]
    (default: NaN)."""
    pose = np.array(origin, dtype=np.float64)
    cur = np.full((len(rig), 7), np.nan) if targets is None else np.array(targets, dtype=np.float64)
    poses, tgts = [], []
    for r in np.asarray(readings, dtype=np.float64):
        pose, t = stream_step(pose, r, rig, inc)
        cur = np.where(np.isnan(t), cur, t)
        poses.append(pose)
        tgts.append(cur)
    return np.array(poses), np.array(tgts)


def record_readings(read, ticks):
    """`ticks` readings of a SpaceMouse reader (anything returning an object with x, y, z, roll, pitch, yaw) as [ticks, 6]."""
    out = np.empty((int(ticks), 6))
    for t in range(int(ticks)):
        v = read()
        out[t] = (v.x, v.y, v.z, v.roll, v.pitch, v.yaw)
    return out


def to_struct(rig, ticks, nb, nb_origin, increment=INCREMENT, loop=False):
    """-> _lib.TeleopStream of a rig (one follower per device, targets order)."""
    if len(rig) > _lib.MAX_DEV:
        raise ValueError(f"a rig holds at most {_lib.MAX_DEV} followers, got {len(rig)}")
    d = _lib.TeleopStream()
    d.ticks, d.nb, d.nb_origin, d.loop, d.increment = int(ticks), int(nb), int(nb_origin), int(bool(loop)), float(increment)
    for k in range(_lib.MAX_DEV):
        d.off_quat[k][0] = 1.0
    for k, f in enumerate(rig):
        d.kind[k], d.heading_offset[k] = int(f["kind"]), float(f["heading_offset"])
        for i in range(3):
            d.off_xyz[k][i] = float(f["off_xyz"][i])
        for i in range(4):
            d.off_quat[k][i] = float(f["off_quat"][i])
    return d
