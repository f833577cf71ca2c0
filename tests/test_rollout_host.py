"""Closed loops on the GPU, the part that needs no GPU: the three exports of the rollout are declared in include/irlosc.h, fall under the
version script's pattern and are bound by _lib.py (tests/test_abi.py then holds `nm -D` against the header)."""
import os
import re

import pytest

from conftest import ROOT
from irl_control_amd import _lib

NEW = ("irlosc_set_plant", "irlosc_rollout_from_q", "irlosc_download_q")


def _header():
    with open(os.path.join(ROOT, "include", "irlosc.h")) as f:
        return f.read()


def test_header_declares_the_rollout_exports():
    h = _header()
    for name in NEW:
        assert re.search(r"IRLOSC_API\s+int\s+" + name + r"\s*\(", h), name
    m = re.search(r"typedef struct irlosc_plant \{(.*?)\} irlosc_plant;", h, flags=re.S)
    assert m, "struct irlosc_plant"
    fields = re.findall(r"(double|uint32_t)\s+(\w+);", m.group(1))
    assert fields == [("double", "dt"), ("double", "damping"), ("uint32_t", "ctrl_mask"), ("uint32_t", "reserved")]
    assert [f[0] for f in _lib.Plant._fields_] == [f[1] for f in fields]
    assert re.search(r"#define\s+IRLOSC_ABI_VERSION\s+3\b", h)      # additive exports: the version stays


def test_version_script_and_binding_list_them():
    with open(os.path.join(ROOT, "irl_control_amd", "csrc", "irlosc.map")) as f:
        assert re.search(r"global:\s*irlosc_\*;", f.read())      # the pattern covers every irlosc_* entry point
    for name in NEW:
        assert name in _lib.EXPORTS


@pytest.mark.skip(reason="irlosc_set_plant validates against a context, and a context needs a HIP device (the library has no CPU "
                         "fallback and no stub): its argument checks are tested on the GPU in tests/test_rollout.py")
def test_set_plant_argument_validation():
    pass
