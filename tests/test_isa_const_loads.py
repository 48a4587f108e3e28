"""The plain single-step kernel issues the scalar loads of its physics constants and of the wind AHEAD of its 14 row loads and
waits for them only after the last row load (profiles/const_block.md: 0.29 us per launch at 2^20 drones).  Read from a fresh
gfx950 disassembly, like tests/test_isa_claims.py; no GPU needed."""
import os
import re
import shutil
import sys

import pytest

from conftest import REPO

sys.path.insert(0, os.path.join(REPO, "tools"))

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")


def test_constant_loads_go_out_ahead_of_the_row_loads(tmp_path):
    import hot_kernel_isa as h
    asm, _ = h.disassemble(str(tmp_path / "fpv.s"))
    bodies = h.kernel_bodies(asm)
    name = next(n for n in bodies if h.HOT["plain single-step kernel fpv_drone_step_kernel<false,false,false,false>"] in n)
    block = h.load_block(bodies[name])
    rows = [k for k, ln in enumerate(block) if re.match(r"global_load_dword v\d+, v\[\d+:\d+\], off", ln)]
    scalar = [k for k, ln in enumerate(block) if ln.startswith("s_load_")]
    assert len(rows) == 14
    # the constants the physics reads (two dwordx16 among them) and the wind (the dwordx4 at the end of the argument)
    assert sum(1 for k in scalar if block[k].startswith("s_load_dwordx16")) == 2 and len(scalar) >= 4
    assert max(scalar) < rows[0], "a scalar load of a constant is issued behind a row load"
    assert block[max(scalar)].startswith("s_load_dwordx4"), "the wind goes out after the constants (its dead fourth dword must not be reused by one of them)"
    # no wait stands between the first load of the block and the last row load
    assert not any(ln.startswith("s_waitcnt") for ln in block[:rows[-1]])
    assert "lgkmcnt(0)" in block[-1] or any("lgkmcnt(0)" in ln for ln in bodies[name][bodies[name].index(block[-1]):][:40])
