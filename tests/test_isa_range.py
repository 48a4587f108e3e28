"""The kernel of the range sensor (csrc/fpv_range.hip) against the compiler's own resource report of a FRESH gfx950 build - no GPU
needed: one kernel, no scratch, no spilled register, no accumulation registers (no MFMA), and the registers and occupancy
DESIGN 3.7 quotes.  Only the report (-Rpass-analysis=kernel-resource-usage) and the kernel's name are read."""
import os
import re
import shutil
import sys

import pytest

from conftest import REPO

sys.path.insert(0, os.path.join(REPO, "tools"))
SRC = os.path.join(REPO, "fpyv_amd", "csrc", "fpv_range.hip")
pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")

KERNELS = {"fpv_range_scan_kernel": "fpv_range_scan_kernelE"}


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    import hot_kernel_isa as h
    _, rem = h.disassemble(str(tmp_path_factory.mktemp("isa") / "range.s"), src=SRC)
    res = h.resources(rem)
    agpr, cur = {}, None
    for ln in rem.splitlines():
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            cur = m.group(1)
        m = re.search(r"remark:\s+AGPRs: (\d+)", ln)
        if m and cur:
            agpr[cur] = int(m.group(1))
    return res, agpr


def test_one_kernel_without_scratch_spill_or_accumulation_registers(report):
    res, agpr = report
    design = open(os.path.join(REPO, "DESIGN.md"), encoding="utf-8").read()
    assert "### 3.7 Range sensor" in design and "One kernel, `fpv_range_scan_kernel`" in design
    assert len(res) == 1, sorted(res)
    for pat in KERNELS.values():
        assert sum(pat in n for n in res) == 1, pat
    for name, r in res.items():
        assert r.get("scratch", 0) == 0 and r.get("sspill", 0) == 0 and r.get("vspill", 0) == 0, (name, r)
        assert r.get("lds", 0) == 0, (name, r)
        assert agpr.get(name, 0) == 0, name


def test_registers_and_occupancy_are_what_design_quotes(report):
    res, _ = report
    design = open(os.path.join(REPO, "DESIGN.md"), encoding="utf-8").read()
    for title, pat in KERNELS.items():
        r = res[next(n for n in res if pat in n)]
        row = f"| `{title}` | {r['vgpr']} | {r['occ']} |"
        assert row in design, f"DESIGN 3.7 does not quote {row}"
