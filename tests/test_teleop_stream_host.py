"""The teleoperation stream on the GPU, the part that needs no GPU: the three exports are declared in include/irlosc.h with their
constants and struct irlosc_teleop_stream, fall under the version script's pattern, are bound by _lib.py with a struct of the header's
layout, and the ABI version stays 3 (tests/test_abi.py then holds `nm -D` against the header); and teleop.stream_step -- the NumPy
mirror the GPU tests hold the kernel to -- against the reference-pinned caller loop (examples/teleop_loops.py::space_mouse_loop)."""
import ctypes as C
import fnmatch
import os
import re
import sys
import types

import numpy as np

from conftest import ROOT
from irl_control_amd import _lib, synth, teleop
from irl_control_amd.input_devices import SpaceMouse
from irl_control_amd.targets import Target

if os.path.join(ROOT, "examples") not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, "examples"))

import teleop_loops as tl                                # noqa: E402

NEW = ("irlosc_set_teleop_stream", "irlosc_download_teleop_state", "irlosc_download_targets")
CTYPES = {"int32_t": C.c_int32, "double": C.c_double}
DIMS = {"IRLOSC_MAX_DEV": _lib.MAX_DEV, "3": 3, "4": 4}


def _header():
    with open(os.path.join(ROOT, "include", "irlosc.h")) as f:
        return f.read()


def test_header_declares_the_stream_exports():
    h = _header()
    for name in NEW:
        assert re.search(r"IRLOSC_API\s+int\s+" + name + r"\s*\(", h), name
    assert re.search(r"#define\s+IRLOSC_MAX_STREAM_TICKS\s+16384\b", h) and _lib.MAX_STREAM_TICKS == 16384
    for name, val in (("NONE", 0), ("RIGID", 1), ("HEADING", 2)):
        assert re.search(r"#define\s+IRLOSC_TELEOP_" + name + r"\s+" + str(val) + r"\b", h), name
        assert getattr(_lib, "TELEOP_" + name) == val
    assert re.search(r"#define\s+IRLOSC_ABI_VERSION\s+3\b", h) and _lib.ABI_VERSION == 3      # additive exports: the version stays


def test_version_script_and_binding_list_them():
    with open(os.path.join(ROOT, "irl_control_amd", "csrc", "irlosc.map")) as f:
        pats = re.search(r"global:(.*?);\s*local:", f.read(), flags=re.S).group(1).replace(";", " ").split()
    for name in NEW:
        assert any(fnmatch.fnmatchcase(name, p) for p in pats), (name, pats)
        assert name in _lib.EXPORTS


def test_stream_struct_matches_header_layout():
    """The binding's struct field by field against the header's: names, order, element types, array shapes -- and the size a C compiler
    gives that layout (natural alignment: 4 int32 | double | 4 int32 | 4 x 3 double | 4 x 4 double | 4 double)."""
    m = re.search(r"typedef struct irlosc_teleop_stream \{(.*?)\} irlosc_teleop_stream;", _header(), flags=re.S)
    assert m, "struct irlosc_teleop_stream"
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = re.findall(r"(int32_t|double)\s+(\w+)((?:\[\w+\])*);", body)
    assert fields == [("int32_t", "ticks", ""), ("int32_t", "nb", ""), ("int32_t", "nb_origin", ""), ("int32_t", "loop", ""),
                      ("double", "increment", ""), ("int32_t", "kind", "[IRLOSC_MAX_DEV]"), ("double", "off_xyz", "[IRLOSC_MAX_DEV][3]"),
                      ("double", "off_quat", "[IRLOSC_MAX_DEV][4]"), ("double", "heading_offset", "[IRLOSC_MAX_DEV]")]

    def ctype(t, dims):
        out = CTYPES[t]
        for d in reversed(re.findall(r"\[(\w+)\]", dims)):      # C's a[X][Y] is X arrays of Y
            out = out * DIMS[d]
        return out
    mirror = type("Mirror", (C.Structure,), {"_fields_": [(n, ctype(t, dims)) for t, n, dims in fields]})
    assert [f[0] for f in _lib.TeleopStream._fields_] == [f[1] for f in fields]
    assert C.sizeof(_lib.TeleopStream) == C.sizeof(mirror) == 16 + 8 + 16 + 96 + 128 + 32
    for name, _ in mirror._fields_:
        assert getattr(_lib.TeleopStream, name).offset == getattr(mirror, name).offset, name
        assert getattr(_lib.TeleopStream, name).size == getattr(mirror, name).size, name


def test_space_mouse_rig_follows_the_layout():
    rig = teleop.space_mouse_rig(synth.make_layout("k13"))          # ur5right, ur5left, base
    assert [f["kind"] for f in rig] == [teleop.RIGID, teleop.RIGID, teleop.HEADING]
    assert list(rig[0]["off_xyz"]) == [0.2, 0.0, 0.0] and list(rig[0]["off_quat"]) == [1.0, 0.0, 0.0, 0.0]
    assert list(rig[1]["off_xyz"]) == [-0.2, 0.0, 0.0] and np.allclose(rig[1]["off_quat"], [0.0, 0.0, 0.0, 1.0], atol=1e-16)
    assert abs(float(rig[1]["off_quat"] @ rig[1]["off_quat"]) - 1.0) <= 1e-12
    assert rig[2]["heading_offset"] == -np.pi / 2
    assert [f["kind"] for f in teleop.space_mouse_rig(synth.make_layout("r6"))] == [teleop.RIGID]      # devices the layout lacks: dropped
    assert [f["kind"] for f in teleop.space_mouse_rig(synth.make_layout("br7"))] == [teleop.HEADING, teleop.RIGID]
    d = teleop.to_struct(rig, 48, 1, 1)
    assert (d.ticks, d.nb, d.nb_origin, d.loop, d.increment) == (48, 1, 1, 0, 0.0015)
    assert list(d.kind) == [1, 1, 2, 0] and list(d.off_quat[3]) == [1.0, 0.0, 0.0, 0.0]


class _Recorder:
    """A controller stub for space_mouse_loop: records the pose7 of every target it is handed and drives nothing."""

    def __init__(self):
        self.targets = []

    def generate(self, targets):
        self.targets.append(np.array([t.pose7() for t in targets.values()]))
        return [], []


def _sim_stub():
    data = types.SimpleNamespace(ctrl=np.zeros(1), set_mocap_pos=lambda *a: None, set_mocap_quat=lambda *a: None)
    return types.SimpleNamespace(data=data, step=lambda: None)


def test_mirror_follows_the_reference_pinned_loop():
    """teleop.stream_step against teleop_loops.space_mouse_loop on space_mouse_stream(5, 200): the loop goes mat2euler -> set_abg ->
    euler2quat where the mirror multiplies quaternions, so target quaternions agree as rotations -- min(|q - q'|, |q + q'|) <= 1e-14 --
    and xyz within 1e-14 (observed: 2.8e-16 / 8.9e-16); the integrated pose is SpaceMouse.update_state's bit for bit."""
    T = 200
    origin = list(teleop.ORIGIN)
    rec = _Recorder()
    out = tl.space_mouse_loop(None, rec, Target, _sim_stub(), SpaceMouse(origin, reader=tl.space_mouse_stream(5, T)), T)
    ref = np.array(rec.targets)                                     # [T, 3, 7]: ur5right, ur5left, base
    readings = teleop.record_readings(tl.space_mouse_stream(5, T), T)
    rig = teleop.space_mouse_rig(synth.make_layout("k13"))
    poses, tgts = teleop.stream_run(origin, readings, rig, targets=np.tile([0.0, 0, 0, 1, 0, 0, 0], (3, 1)))
    assert np.array_equal(poses, out["pose"])
    assert np.abs(poses[:, 3:]).max() <= np.pi
    dxyz = np.abs(tgts[:, :, :3] - ref[:, :, :3]).max()
    dq = np.minimum(np.abs(tgts[:, :, 3:] - ref[:, :, 3:]).max(axis=2), np.abs(tgts[:, :, 3:] + ref[:, :, 3:]).max(axis=2)).max()
    print(f"mirror vs the loop over {T} ticks: max |xyz| {dxyz:.3g}, quaternions as rotations {dq:.3g}")
    assert dxyz <= 1e-14 and dq <= 1e-14, (dxyz, dq)
    assert np.all(tgts[:, 2, :3] == 0.0)                            # HEADING leaves the xyz words alone


def test_stream_step_marks_the_words_it_does_not_write():
    rig = [teleop.follower(), teleop.follower(teleop.HEADING, heading_offset=0.25), teleop.follower(teleop.RIGID, (0.0, 0.1, 0.0))]
    pose, tgt = teleop.stream_step(teleop.ORIGIN, [1.0, -2.0, 3.0, 4.0, -5.0, 6.0], rig, 0.01)
    assert np.all(np.isnan(tgt[0])) and np.all(np.isnan(tgt[1, :3])) and np.all(np.isfinite(tgt[1, 3:])) and np.all(np.isfinite(tgt[2]))
    assert np.allclose(pose, [0.01, 0.48, 0.53, 0.04, 0.05, -0.06], atol=1e-15)
    assert abs(tgt[1, 3] - np.cos((np.arctan2(pose[1], pose[0]) + 0.25) / 2)) <= 1e-16
