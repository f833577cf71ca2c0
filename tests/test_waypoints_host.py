"""Waypoint paths on the GPU, the part that needs no GPU: the two exports are declared in include/irlosc.h with IRLOSC_MAX_WAYPOINTS
and struct irlosc_waypoints, fall under the version script's pattern, are bound by _lib.py with a struct of the header's layout, and
the ABI version stays 3 (tests/test_abi.py then holds `nm -D` against the header)."""
import ctypes as C
import fnmatch
import os
import re

from conftest import ROOT
from irl_control_amd import _lib

NEW = ("irlosc_set_waypoints", "irlosc_download_waypoint_state")
CTYPES = {"int32_t": C.c_int32, "uint32_t": C.c_uint32, "double": C.c_double, "uint8_t": C.c_uint8}


def _header():
    with open(os.path.join(ROOT, "include", "irlosc.h")) as f:
        return f.read()


def test_header_declares_the_waypoint_exports():
    h = _header()
    for name in NEW:
        assert re.search(r"IRLOSC_API\s+int\s+" + name + r"\s*\(", h), name
    assert re.search(r"#define\s+IRLOSC_MAX_WAYPOINTS\s+64\b", h)
    assert _lib.MAX_WAYPOINTS == 64
    assert re.search(r"#define\s+IRLOSC_ABI_VERSION\s+3\b", h) and _lib.ABI_VERSION == 3      # additive exports: the version stays


def test_version_script_and_binding_list_them():
    with open(os.path.join(ROOT, "irl_control_amd", "csrc", "irlosc.map")) as f:
        pats = re.search(r"global:(.*?);\s*local:", f.read(), flags=re.S).group(1).replace(";", " ").split()
    for name in NEW:
        assert any(fnmatch.fnmatchcase(name, p) for p in pats), (name, pats)
        assert name in _lib.EXPORTS


def test_waypoints_struct_matches_header_layout():
    """The binding's struct field by field against the header's: names, order, element types, array lengths -- and the size a C compiler
    gives that layout (natural alignment: 4 int32 | 4 double | 4 uint8 | int32 = 16 + 32 + 4 + 4)."""
    m = re.search(r"typedef struct irlosc_waypoints \{(.*?)\} irlosc_waypoints;", _header(), flags=re.S)
    assert m, "struct irlosc_waypoints"
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = re.findall(r"(int32_t|uint32_t|double|uint8_t)\s+(\w+)(?:\[(\w+)\])?;", body)
    assert fields == [("int32_t", "count", "IRLOSC_MAX_DEV"), ("double", "threshold", "IRLOSC_MAX_DEV"),
                      ("uint8_t", "loop", "IRLOSC_MAX_DEV"), ("int32_t", "nb", "")]
    mirror = type("Mirror", (C.Structure,), {"_fields_": [(n, CTYPES[t] * _lib.MAX_DEV if dim else CTYPES[t]) for t, n, dim in fields]})
    assert [f[0] for f in _lib.Waypoints._fields_] == [f[1] for f in fields]
    assert C.sizeof(_lib.Waypoints) == C.sizeof(mirror) == 16 + 32 + 4 + 4
    for name, _ in mirror._fields_:
        assert getattr(_lib.Waypoints, name).offset == getattr(mirror, name).offset, name
        assert getattr(_lib.Waypoints, name).size == getattr(mirror, name).size, name
