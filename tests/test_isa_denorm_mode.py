"""The floating-point mode the device branch of fpv_sqrt_flushed relies on (csrc/fpv_math.h): its error terms are exact only while
fp32 denormals are kept, and the host lane model keeps them.  Every kernel of all four translation units must ask for that in its
kernel descriptor - FLOAT_DENORM_MODE_32 = 3: denormal sources and results preserved - as must the 16/64-bit field the fp16
conversions read.  A FRESH gfx950 build at the shipped flags, no GPU needed; only the descriptors' mode fields are read."""
import os
import re
import shutil
import sys
from concurrent.futures import ThreadPoolExecutor

import pytest

from conftest import REPO

sys.path.insert(0, os.path.join(REPO, "tools"))
pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")

UNITS = ("fpv_hip.hip", "fpv_phys.hip", "fpv_gate.hip", "fpv_range.hip")


def descriptors(asm):
    """{kernel name: {field: value}} of every .amdhsa_kernel block of a listing"""
    out = {}
    for m in re.finditer(r"^\s*\.amdhsa_kernel (\S+)\n(.*?)^\s*\.end_amdhsa_kernel", asm, re.M | re.S):
        out[m.group(1)] = {k: int(v, 0) for k, v in re.findall(r"\.amdhsa_(\w+) (\S+)", m.group(2)) if re.fullmatch(r"(0x)?[0-9a-fA-F]+", v)}
    return out


def test_every_kernel_keeps_fp32_denormals(tmp_path):
    import __graft_entry__ as entry
    import hot_kernel_isa as h
    assert sorted(os.path.basename(s) for s in entry.HIP_SRCS) == sorted(UNITS), "a translation unit this test does not read"
    with ThreadPoolExecutor(len(UNITS)) as pool:
        listings = list(pool.map(lambda u: h.disassemble(str(tmp_path / (u + ".s")), src=os.path.join(REPO, "fpyv_amd", "csrc", u))[0], UNITS))
    total = 0
    for unit, asm in zip(UNITS, listings):
        desc = descriptors(asm)
        assert desc and set(desc) == set(h.kernel_bodies(asm)), unit
        for name, d in desc.items():
            assert d["float_denorm_mode_32"] == 3, (unit, name, d["float_denorm_mode_32"])
            assert d["float_denorm_mode_16_64"] == 3, (unit, name, d["float_denorm_mode_16_64"])
            assert d["float_round_mode_32"] == 0 and d["float_round_mode_16_64"] == 0, (unit, name)     # round to nearest even
        total += len(desc)
    assert total >= 42
