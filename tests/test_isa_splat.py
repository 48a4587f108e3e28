"""The kernel of the point-cloud camera (csrc/fpv_splat.hip) against the compiler's own resource report of a FRESH gfx950 build - no
GPU needed: one kernel, no scratch (the object tables travel by value in the kernel argument; the prune indexes them by lane: were
they copied to private memory, scratch would show here), no spilled register, no static LDS (the z-buffer is dynamic: W * H words
asked for at the launch), no accumulation registers (no MFMA), and the registers and occupancy DESIGN 3.13 quotes; the floating-point
mode of its kernel descriptor - fp32 denormals kept, round to nearest even - which the bit identity with the host relies on.  Only
the report (-Rpass-analysis=kernel-resource-usage), the descriptor's mode fields and the kernel's name are read."""
import os
import re
import shutil
import sys

import pytest

from conftest import REPO

sys.path.insert(0, os.path.join(REPO, "tools"))
CSRC = os.path.join(REPO, "fpyv_amd", "csrc")
SRC = os.path.join(CSRC, "fpv_splat.hip")
pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")

KERNELS = {"fpv_splat_kernel": "fpv_splat_kernelE"}


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    import hot_kernel_isa as h
    asm, rem = h.disassemble(str(tmp_path_factory.mktemp("isa") / "splat.s"), src=SRC)
    res = h.resources(rem)
    agpr, cur = {}, None
    for ln in rem.splitlines():
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            cur = m.group(1)
        m = re.search(r"remark:\s+AGPRs: (\d+)", ln)
        if m and cur:
            agpr[cur] = int(m.group(1))
    return res, agpr, asm


def test_one_kernel_without_scratch_spill_static_lds_or_accumulation_registers(report):
    res, agpr, _ = report
    design = open(os.path.join(REPO, "DESIGN.md"), encoding="utf-8").read()
    assert "### 3.13 Point-cloud camera" in design
    assert len(res) == 1, sorted(res)
    for pat in KERNELS.values():
        assert sum(pat in n for n in res) == 1, pat
    for name, r in res.items():
        assert r.get("scratch", 0) == 0 and r.get("sspill", 0) == 0 and r.get("vspill", 0) == 0, (name, r)
        assert r.get("lds", 0) == 0, (name, r)
        assert agpr.get(name, 0) == 0, name


def test_registers_and_occupancy_are_what_design_quotes(report):
    res, _, _ = report
    design = open(os.path.join(REPO, "DESIGN.md"), encoding="utf-8").read()
    for title, pat in KERNELS.items():
        r = res[next(n for n in res if pat in n)]
        row = f"| `{title}` | {r['vgpr']} | {r['sgpr']} | {r['occ']} |"
        assert row in design, f"DESIGN 3.13 does not quote {row}"


def test_the_build_links_this_unit_and_its_descriptor_keeps_fp32_denormals(report):
    import __graft_entry__ as entry
    from test_isa_denorm_mode import descriptors
    assert entry.HIP_SRCS_SPLAT == entry.HIP_SRCS_DETECT + [SRC]           # the nine units the other ISA tests read, and this one
    _, _, asm = report
    desc = descriptors(asm)
    assert len(desc) == 1
    for name, d in desc.items():
        assert d["float_denorm_mode_32"] == 3 and d["float_denorm_mode_16_64"] == 3, (name, d)
        assert d["float_round_mode_32"] == 0 and d["float_round_mode_16_64"] == 0, name
