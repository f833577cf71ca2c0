"""Host side of the F/T sensor feed of the path from joint coordinates (no GPU): the ctypes struct against the header, the default
description for the shipped model, and R_rel = R(ee)^T R(site) -- the constant the library composes with the EE frame -- restated in
NumPy over the rigid-body oracle."""
import ctypes as C

import numpy as np

from irl_control_amd import _lib
from irl_control_amd.rigid_body import DUAL_UR5_EE, RigidBodyModel
from oracle import rigid_body as rb


def test_ft_desc_struct_matches_header_layout():
    # int32 n_sensor, int32 site_body[4], (pad to 8) double site_quat[4][4], int32 ft_force0[4], int32 ft_torque0[4]
    assert _lib.FtDesc.site_quat.offset == 24
    assert _lib.FtDesc.ft_force0.offset == 24 + 128
    assert C.sizeof(_lib.FtDesc) == 24 + 128 + 16 + 16


def test_new_entry_points_are_declared_and_bound():
    for name in ("irlosc_set_ft_sensors", "irlosc_set_sensordata", "irlosc_step_from_q_device"):
        assert name in _lib.EXPORTS


def test_default_ft_desc_of_the_shipped_model():
    model = RigidBodyModel.load("dual_ur5")
    fd = model.ft_desc(["ur5right", "ur5left"])
    assert fd.n_sensor == 18
    assert list(fd.site_body) == [11, 27, -1, -1]
    assert [model.bodies[b]["name"] for b in fd.site_body[:2]] == ["robotiq_85_adapter_link_ur5right", "robotiq_85_adapter_link_ur5left"]
    assert list(fd.ft_force0)[:2] == [0, 6] and list(fd.ft_torque0)[:2] == [3, 9]
    assert list(fd.ft_force0)[2:] == [-1, -1]
    # a device without an F/T sensor in the scene (the stand) has none; another site can be named per device
    fd = model.ft_desc(["base", "ur5right", "ur5left"], sites={"ur5left": "gripper_frame_ur5left"})
    assert list(fd.site_body)[:3] == [-1, 11, 33]
    assert list(fd.ft_force0)[:3] == [-1, 0, 6]


def _r_rel(om, q, ee, site):
    kin = rb.kinematics(om, q)
    R_site = kin["xmat"][site["body"]] @ rb.quat2mat(np.asarray(site["quat"]) / np.linalg.norm(site["quat"]))
    return kin["xmat"][ee].T @ R_site


def test_r_rel_is_constant_over_joint_coordinates():
    """What irlosc_set_ft_sensors precomputes is a constant of the model: R(ee)^T R(site) at random q equals the value at q = 0 to
    1e-14, for the F/T site of each arm (welded to the arm's EE body)."""
    om = rb.Model()
    model = RigidBodyModel.load("dual_ur5")
    rng = np.random.default_rng(7)
    qpos, _ = model.random_state(rng, 32)
    for dev in ("ur5right", "ur5left"):
        ee = om.body_id(DUAL_UR5_EE[dev])
        site = om.site("ft_frame_" + dev)
        R0 = _r_rel(om, np.zeros(om.nj), ee, site)
        assert np.allclose(R0 @ R0.T, np.eye(3), atol=1e-14)
        for q in qpos:
            assert np.abs(_r_rel(om, q, ee, site) - R0).max() <= 1e-14
        # (and the gripper's frame is NOT rigid to the EE: a finger hinge lies between them)
        g = om.site("gripper_frame_" + dev)
        q = qpos[0].copy()
        R1 = _r_rel(om, q, ee, g)
        q[np.nonzero(om.anc[g["body"]] & ~om.anc[ee])[0][0]] += 0.3
        assert np.abs(_r_rel(om, q, ee, g) - R1).max() > 1e-3
