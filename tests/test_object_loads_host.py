"""The weight of the action objects on the host (no GPU): the new ctypes struct and exports against include/irlosc.h, the NumPy mirror
irl_control_amd/object_loads.py::load_wrench on hand-checkable numbers, and the CARRY example's NumPy loop with a mass."""
import ctypes as C
import importlib.util
import os
import re

import numpy as np
import pytest

from irl_control_amd import _lib, object_loads as ol, objects as ob

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = 9.81


def objset(devs=(0,)):
    return ob.ObjectSet(radius=[0.05, 0.05], grippers=[ob.Gripper(dev=d, joint=7, q_close=0.3, q_open=0.1) for d in devs])


def poses(B=1, ndev=2):
    ee = np.zeros((B, ndev, 7))
    ee[:, :, 3] = 1.0
    obj = np.zeros((B, 2, 7))
    obj[:, :, 3] = 1.0
    return ee, obj


def test_the_struct_and_the_exports_against_the_header():
    hdr = open(os.path.join(ROOT, "include", "irlosc.h")).read()
    assert re.search(r"#define IRLOSC_ABI_VERSION\s+3\b", hdr) and _lib.ABI_VERSION == 3      # the exports are additive
    body = hdr[hdr.index("typedef struct irlosc_object_loads {"):hdr.index("} irlosc_object_loads;")]
    fields = re.findall(r"^\s*(?:int32_t|double)\s+(\w+)", body, flags=re.M)
    assert fields == [f[0] for f in _lib.ObjectLoads._fields_] == ["per_robot", "reserved", "gravity"]
    assert C.sizeof(_lib.ObjectLoads) == 2 * 4 + 3 * 8
    assert _lib.ObjectLoads.gravity.offset == 8
    for name in ("irlosc_set_object_loads", "irlosc_download_object_load_state"):
        assert name in _lib.EXPORTS and re.search(rf"^IRLOSC_API int {name}\(", hdr, flags=re.M), name
    # struct irlosc_objects is what it was (tests/test_objects_host.py pins its fields)
    assert "mass" not in hdr[hdr.index("typedef struct irlosc_objects {"):hdr.index("} irlosc_objects;")]
    d = ol.ObjectLoads(mass=[1.0, 2.0], gravity=(0.0, 1.0, -2.0)).to_struct(True)
    assert (d.per_robot, d.reserved, list(d.gravity)) == (1, 0, [0.0, 1.0, -2.0])


def test_the_table_is_shared_unless_a_part_of_it_is_per_robot():
    assert ol.ObjectLoads(mass=[1.0, 2.0]).table(5, 2).shape == (1, 2, 4)
    t = ol.ObjectLoads(mass=np.ones((5, 2)), com=[[0.1, 0.2, 0.3], [0.0, 0.0, 0.0]]).table(5, 2)
    assert t.shape == (5, 2, 4) and np.array_equal(t[3, 0], [1.0, 0.1, 0.2, 0.3])
    assert ol.ObjectLoads(mass=[1.0, 2.0], com=np.zeros((5, 2, 3))).table(5, 2).shape == (5, 2, 4)
    for bad in (dict(mass=[1.0]), dict(mass=np.ones((4, 2))), dict(mass=[1.0, 2.0], com=np.zeros((2, 2)))):
        with pytest.raises(ValueError):
            ol.ObjectLoads(**bad).table(5, 2)


def test_unit_quaternion_no_offset_and_a_unit_arm_give_r_cross_f_exactly():
    """The object one metre along x from the EE, its centre of mass in its origin: F = m g, T = r x F = (0, -r0 F2, 0) = (0, m G, 0)"""
    ee, obj = poses()
    obj[0, 0, :3] = [1.0, 0.0, 0.0]
    holder = np.array([[0, -1]])
    W = ol.load_wrench(ol.ObjectLoads(mass=[2.0, 5.0]), objset(), ee, obj, holder)
    assert W.shape == (1, 1, 6) and np.array_equal(W[0, 0], [0.0, 0.0, -2.0 * G, 0.0, 2.0 * G, 0.0])
    # the holder as word 7 of the log's channel; a centre of mass off the origin, turned with the object (90 degrees about z: x -> y)
    obj8 = np.concatenate([obj, holder[:, :, None].astype(np.float64)], axis=2)
    assert np.array_equal(ol.load_wrench(ol.ObjectLoads(mass=[2.0, 5.0]), objset(), ee, obj8), W)
    obj[0, 0, 3:] = [np.sqrt(0.5), 0.0, 0.0, np.sqrt(0.5)]
    W = ol.load_wrench(ol.ObjectLoads(mass=[2.0, 5.0], com=[[0.5, 0.0, 0.0], [0.0, 0.0, 0.0]]), objset(), ee, obj, holder)[0, 0]
    assert np.allclose(W, [0.0, 0.0, -2.0 * G, -0.5 * 2.0 * G, 1.0 * 2.0 * G, 0.0], atol=1e-15)
    # r is taken from the EE of the gripper's device
    ee[0, 1, :3] = [1.0, 0.0, 0.0]
    assert np.allclose(ol.load_wrench(ol.ObjectLoads(mass=[2.0, 5.0]), objset((1,)), ee, obj, holder)[0, 0, 3:], 0.0, atol=1e-15)


def test_held_against_free_mass_zero_and_a_nan_pose():
    ee, obj = poses(B=4)
    obj[:, :, :3] = [0.3, -0.2, 0.1]
    obj[3, 0, 1] = np.nan                                  # robot 3: a pose that is not finite
    holder = np.array([[0, -1], [-1, -1], [-1, 0], [0, -1]])      # robot 0 holds the plug, 1 nothing, 2 the weightless socket
    W = ol.load_wrench(ol.ObjectLoads(mass=[2.0, 0.0]), objset(), ee, obj, holder)[:, 0]
    assert W[0, 2] == -2.0 * G and W[0, 3] == -0.2 * (-2.0 * G) and W[0, 4] == -(0.3 * (-2.0 * G))
    assert not W[1:].any() and np.all(np.isfinite(W))
    # two grippers: each its own object; the lowest object counts where a hand is named twice
    two = ol.load_wrench(ol.ObjectLoads(mass=[2.0, 3.0]), objset((0, 1)), ee, obj, np.array([[0, 1], [1, 0], [0, 0], [-1, -1]]))
    assert two[0, 0, 2] == -2.0 * G and two[0, 1, 2] == -3.0 * G and two[1, 0, 2] == -3.0 * G and two[1, 1, 2] == -2.0 * G
    assert two[2, 0, 2] == -2.0 * G and not two[2, 1].any() and not two[3].any()
    # per-robot masses
    per = ol.load_wrench(ol.ObjectLoads(mass=[[1.0, 0.0], [2.0, 0.0], [3.0, 0.0], [4.0, 0.0]]), objset(), ee, obj, np.array([[0, -1]] * 4))[:, 0]
    assert np.array_equal(per[:3, 2], [-1.0 * G, -2.0 * G, -3.0 * G]) and not per[3].any()


def test_the_carry_loop_sags_under_the_mass():
    """examples/insertion_carry_resident_headless.py::cpu_loop with the example's mass against the same loop without: both robots hold
    the plug on tick 179 (the grasp falls on ticks 141 and 144), and the fleet's mean EE height is lower with the mass.  (The whole loop,
    1300 ticks: grasp on 141 / 144 either way, release and mate on 1022 / 1031 with 0.2 kg against 1019 / 1028 without, 0.4 mm of sag
    mid-carry; with 0.5 kg 1028 / 1037 and 1.0 mm.)"""
    spec = importlib.util.spec_from_file_location("insertion_carry", os.path.join(ROOT, "examples", "insertion_carry_resident_headless.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    T = 180
    light = ex.cpu_loop(robots=2, ticks=T, verbose=False)
    heavy = ex.cpu_loop(robots=2, ticks=T, verbose=False, mass=ex.MASS)
    assert ex.MASS > 0.0
    assert np.all(light["holder_log"][-1] == 0) and np.all(heavy["holder_log"][-1] == 0)
    assert not light["load_log"].any() and np.all(heavy["load_log"][-1, :, 2] == ex.MASS * -9.81)
    assert not heavy["load_log"][:141].any()
    assert heavy["ee_log"][-1, :, 2].mean() < light["ee_log"][-1, :, 2].mean()
