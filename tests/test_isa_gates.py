"""The kernels of gate courses (csrc/fpv_gate.hip) against the compiler's own resource report of a FRESH gfx950 build - no GPU
needed: five kernels, no scratch, no spilled register, no accumulation registers (no MFMA), the plain single-step kernel at the
headline kernel's 6 waves per SIMD or better, and the registers and occupancy DESIGN 3.6 quotes.  Only the report
(-Rpass-analysis=kernel-resource-usage) and the kernels' names are read."""
import os
import re
import shutil
import sys

import pytest

from conftest import REPO

sys.path.insert(0, os.path.join(REPO, "tools"))
SRC = os.path.join(REPO, "fpyv_amd", "csrc", "fpv_gate.hip")
pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")

KERNELS = {"fpv_drone_step_gate_kernel": "fpv_drone_step_gate_kernelE",
           "fpv_drone_rollout_gate_kernel<0,0>": "fpv_drone_rollout_gate_kernelILb0ELb0EE",
           "fpv_drone_rollout_gate_kernel<0,1>": "fpv_drone_rollout_gate_kernelILb0ELb1EE",
           "fpv_drone_rollout_gate_kernel<1,0>": "fpv_drone_rollout_gate_kernelILb1ELb0EE",
           "fpv_gate_reset_kernel": "fpv_gate_reset_kernelE"}


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    import hot_kernel_isa as h
    _, rem = h.disassemble(str(tmp_path_factory.mktemp("isa") / "gate.s"), src=SRC)
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


def test_five_kernels_without_scratch_spill_or_accumulation_registers(report):
    res, agpr = report
    assert len(res) == 5, sorted(res)
    for pat in KERNELS.values():
        assert sum(pat in n for n in res) == 1, pat
    for name, r in res.items():
        assert r.get("scratch", 0) == 0 and r.get("sspill", 0) == 0 and r.get("vspill", 0) == 0, (name, r)
        assert agpr.get(name, 0) == 0, name


def test_registers_and_occupancy_are_what_design_quotes(report):
    res, _ = report
    design = open(os.path.join(REPO, "DESIGN.md"), encoding="utf-8").read()
    assert "### 3.6 Gate courses" in design
    for title, pat in KERNELS.items():
        r = res[next(n for n in res if pat in n)]
        row = f"| `{title}` | {r['vgpr']} | {r['occ']} |"
        assert row in design, f"DESIGN 3.6 does not quote {row}"
    plain = res[next(n for n in res if KERNELS["fpv_drone_step_gate_kernel"] in n)]
    assert plain["occ"] >= 6                  # the headline single-step kernel's occupancy (6 waves per SIMD) is kept
    assert plain.get("lds", 0) in (0, 4096)   # the descriptor table: gathered from global memory, or the workgroup's 4 KiB copy
