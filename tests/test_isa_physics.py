"""The kernels of per-drone physics (csrc/fpv_phys.hip) against a FRESH gfx950 disassembly - no GPU needed: eight kernels, no
scratch, no spilled register, no MFMA, the table loads of the single-step kernels inside the load block, and the registers and
occupancy DESIGN 3.5 quotes.  tools/hot_kernel_isa.py with the source file as its argument is the same code."""
import os
import re
import shutil
import sys

import pytest

from conftest import REPO

sys.path.insert(0, os.path.join(REPO, "tools"))
SRC = os.path.join(REPO, "fpyv_amd", "csrc", "fpv_phys.hip")
pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    import hot_kernel_isa as h
    asm, rem = h.disassemble(str(tmp_path_factory.mktemp("isa") / "phys.s"), src=SRC)
    return h, h.kernel_bodies(asm), h.resources(rem)


def _kernel(bodies, family, noise, obj):
    return next(n for n in bodies if f"{family}ILb{noise}ELb{obj}EE" in n)


def test_eight_kernels_without_scratch_spill_or_mfma(isa):
    h, bodies, res = isa
    assert len(bodies) == 8
    assert sum("fpv_drone_step_phys_kernel" in n for n in bodies) == 4 and sum("fpv_drone_rollout_phys_kernel" in n for n in bodies) == 4
    for name, body in bodies.items():
        c, r = h.counts(body), res[name]
        assert c["scratch_flat_buffer"] == 0 and c["mfma"] == 0 and c["sgpr_spill_lane_ops"] == 0, name
        assert r.get("scratch", 0) == 0 and r.get("sspill", 0) == 0 and r.get("vspill", 0) == 0, (name, r)


@pytest.mark.parametrize("noise,obj", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_single_step_table_loads_are_issued_in_the_load_block(isa, noise, obj):
    """Every load of the lane - sticks, 14 state rows, 11 table rows and the two ground rows behind their wave-uniform test -
    is issued before the first s_waitcnt that follows the first of them: nothing is waited for between the lane's first load
    and its last table load (the six leading scalars are preloaded into SGPRs; the ground test reads one of them)."""
    h, bodies, _ = isa
    body = bodies[_kernel(bodies, "fpv_drone_step_phys_kernel", noise, obj)]
    start = 0
    if noise:               # the staging of the noise table ends with the workgroup barrier; the lane's own loads begin after it
        start = next(k for k, ln in enumerate(body) if ln.startswith("s_barrier")) + 1
    first = next(k for k in range(start, len(body)) if body[k].startswith("global_load_dword "))
    wait = next(k for k in range(first, len(body)) if body[k].startswith("s_waitcnt"))
    block = body[first:wait]
    rows = [ln for ln in block if ln.startswith("global_load_dword ")]
    # 4 SoA stick loads (the row layout's one dwordx4 is the other arm of a uniform branch) + 14 state rows + 13 table rows
    assert len(rows) == 4 + 14 + 13, (len(rows), block)
    if not obj:             # the two ground rows sit behind a scalar test of the preloaded n_start word, inside the block
        k = max(i for i, ln in enumerate(block) if ln.startswith("global_load_dword "))
        assert any(ln.startswith("s_cbranch_scc") for ln in block[:k]) and any(ln.startswith(("s_cmp_", "s_bitcmp")) for ln in block[:k])


def test_registers_and_occupancy_are_what_design_quotes(isa):
    h, bodies, res = isa
    design = open(os.path.join(REPO, "DESIGN.md"), encoding="utf-8").read()
    assert "### 3.5 Per-drone physics" in design and "+ 8 in `fpv_phys.hip`" in design and "42 kernels" in design
    quoted = 0
    for family in ("fpv_drone_step_phys_kernel", "fpv_drone_rollout_phys_kernel"):
        for noise in (0, 1):
            for obj in (0, 1):
                r = res[_kernel(bodies, family, noise, obj)]
                row = f"| `{family}<{noise},{obj}>` | {r['vgpr']} | {r['occ']} |"
                assert row in design, f"DESIGN 3.5 does not quote {row}"
                quoted += 1
    assert quoted == 8
    plain = res[_kernel(bodies, "fpv_drone_step_phys_kernel", 0, 0)]
    assert plain["occ"] >= 6                  # the plain single-step kernel's occupancy (73 VGPRs / 6 waves) is kept
