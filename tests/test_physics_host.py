"""Per-drone physics on the host (include/fpv_abi.h "Per-drone physics") - no GPU needed: fpv_physics_derive gives a drone the
constants fpv_create would narrow from its parameters, fpv_physics_sample is the documented Philox draw, the exports exist, the
ABI number and both structs are what they were, and fpv_hip.hip alone still builds into a library that says what it lacks."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import REPO
from fpyv_amd import _lib, load_params, physics
from oracle import philox
from physics_sets import dealt, inputs_of, parameter_sets

FPV_EINVAL, FPV_EPARAM = -1, -5
NEW = ("fpv_physics_rows", "fpv_physics_derive", "fpv_physics_sample", "fpv_set_physics", "fpv_get_physics")
RATE_LIM, OMKR, OMKT, DK3, DK2, DK1, DK0, KDX, KDY, KDZ, INV_MASS, GK, GC = range(13)


def _base():
    return load_params(fps=1000, ground=True, ground_damping=3.0)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_derive_equals_the_homogeneous_constants():
    base = _base()
    sets = parameter_sets(base)
    assert len(sets) == 8
    cb = _lib.pack_params(base)
    assert _lib.lib().fpv_physics_rows() == 13 == _lib.FPV_PHYS_ROWS
    table = physics.derive(cb, np.stack([inputs_of(p) for p in sets]))
    for k, p in enumerate(sets):
        own = physics.derive(_lib.pack_params(p), np.full((1, 10), np.nan))          # the set as the base, NaN = "the base value"
        assert np.array_equal(_bits(table[:, k]), _bits(own[:, 0])), k
        # float64 restatement, narrowed once
        h = 50.0
        c3, c2, c1, c0 = (float(x) for x in p.thrust_poly)
        kt = p.thrust_transition_rate
        want = {INV_MASS: 1.0 / p.mass,
                DK3: kt * (c3 * h ** 3), DK2: kt * (3 * c3 * h ** 3 + c2 * h ** 2),
                DK1: kt * (3 * c3 * h ** 3 + 2 * c2 * h ** 2 + c1 * h), DK0: kt * (c3 * h ** 3 + c2 * h ** 2 + c1 * h + c0)}
        for i in range(3):
            want[KDX + i] = 0.5 * p.drag_coefficients[i] * p.air_density * p.cross_section_areas[i] / p.mass
        for r, v in want.items():
            # the same float64 expression, narrowed once
            assert _bits(table[r, k]) == _bits(np.float32(v)), (k, r, table[r, k], v)
        assert table[RATE_LIM, k] == np.float32(p.max_rates * p.rates_transition_rate)
        assert table[OMKR, k] == np.float32(1.0 - p.rates_transition_rate) and table[OMKT, k] == np.float32(1.0 - kt)
        assert table[GK, k] == np.float32(p.ground_spring / p.mass) and table[GC, k] == np.float32(p.ground_damping / p.mass)
    assert len({table[:, k].tobytes() for k in range(8)}) == 8


def test_nan_cells_keep_the_base_value_and_bad_cells_are_refused():
    base = _base()
    cb = _lib.pack_params(base)
    L = _lib.lib()
    ref = physics.derive(cb, None, 1)[:, 0]
    sets = np.full((6, 10), np.nan)
    sets[2, 0] = 2.0 * base.mass                                 # only the mass moved: the mass rows move, the others stay
    rows = physics.derive(cb, sets)
    for i in (0, 1, 3, 4, 5):
        assert np.array_equal(_bits(rows[:, i]), _bits(ref))
    moved = [KDX, KDY, KDZ, INV_MASS, GK, GC]
    assert all(rows[r, 2] != ref[r] for r in moved) and all(rows[r, 2] == ref[r] for r in range(13) if r not in moved)
    for bad_cell, value in (((3, 0), 0.0), ((4, 0), -1.0), ((1, 6), np.inf), ((5, 9), -np.inf)):
        s = sets.copy()
        s[bad_cell] = value
        out = np.empty((13, 6), np.float32)
        assert L.fpv_physics_derive(C.byref(cb), 6, s.ctypes.data, out.ctypes.data, 6) == FPV_EPARAM
        assert f"drone {bad_cell[0]}:".encode() in L.fpv_last_error(), L.fpv_last_error()
    with pytest.raises(_lib.FpvError, match="drone 3"):
        s = sets.copy()
        s[3, 0] = 0.0
        physics.derive(cb, s)
    out = np.empty((13, 4), np.float32)
    assert L.fpv_physics_derive(C.byref(cb), 6, sets.ctypes.data, out.ctypes.data, 4) == FPV_EINVAL      # out_ld < n


RANGES = dict(mass=(0.7, 1.4), thrust=(0.8, 1.25), drag=(0.5, 2.0), rates_lag=(0.6, 1.1), thrust_lag=(0.9, 1.5))


def test_sampling_is_keyed_by_seed_and_global_id_only():
    base = _base()
    cb = _lib.pack_params(base)
    N, seed, off = 4096, 0xFEED_0000_BEEF, (1 << 33) + 77
    whole = physics.sample(cb, seed, off, N, **RANGES)
    halves = np.concatenate([physics.sample(cb, seed, off, N // 2, **RANGES), physics.sample(cb, seed, off + N // 2, N // 2, **RANGES)])
    assert np.array_equal(whole, halves)
    b = physics.base_inputs(cb)
    lo = np.array([RANGES["mass"][0]] + [RANGES["thrust"][0]] * 4 + [RANGES["drag"][0]] * 3 + [RANGES["rates_lag"][0], RANGES["thrust_lag"][0]])
    hi = np.array([RANGES["mass"][1]] + [RANGES["thrust"][1]] * 4 + [RANGES["drag"][1]] * 3 + [RANGES["rates_lag"][1], RANGES["thrust_lag"][1]])
    f = whole / b
    assert np.all(f >= lo - 1e-12) and np.all(f <= hi + 1e-12)
    assert np.allclose(f[:, 1], f[:, 2], rtol=1e-14) and np.allclose(f[:, 1], f[:, 4], rtol=1e-14)      # ONE factor for the whole cubic
    assert np.abs(f[:, 5] - f[:, 6]).min() > 0                                                           # one factor per drag axis
    # the words: Philox4x32-7, key = seed, counter = (gid lo, gid hi ^ (block << 28), "PHYS", 0)
    ids = np.array([0, 1, 2, 1000, N - 1])
    gid = (ids + off).astype(np.uint64)
    key = np.array([[seed & 0xFFFFFFFF, seed >> 32]] * len(ids), dtype=np.uint32)
    for block, cols in ((0, (0, 1, 8, 9)), (1, (5, 6, 7))):
        ctr = np.stack([gid & np.uint64(0xFFFFFFFF), (gid >> np.uint64(32)) ^ np.uint64(block << 28),
                        np.full(len(ids), 0x53594850, np.uint64), np.zeros(len(ids), np.uint64)], axis=-1).astype(np.uint32)
        w = philox.philox4x32(ctr, key, rounds=7)
        for word, c in enumerate(cols):
            u = (w[:, word] >> np.uint32(8)).astype(np.float64) * 2.0 ** -24
            assert np.allclose(f[ids, c], lo[c] + (hi[c] - lo[c]) * u, rtol=0, atol=1e-13), (block, c)
    other = physics.sample(cb, seed + 1, off, N, **RANGES)
    assert np.mean(other[:, 0] != whole[:, 0]) > 0.99
    means = f.mean(0)
    assert np.all(np.abs(means - (lo + hi) / 2) < 5 * (hi - lo) / np.sqrt(12 * N))
    r = np.ones((10, 2))
    r[0, 1] = np.inf
    out = np.empty((4, 10))
    assert _lib.lib().fpv_physics_sample(C.byref(cb), 1, 0, 4, r.ctypes.data, out.ctypes.data) == FPV_EPARAM


def test_exports_and_the_abi_are_what_they_were():
    hdr = open(os.path.join(REPO, "include", "fpv_abi.h")).read()
    L = _lib.lib()
    for name in NEW:
        assert name in _lib.EXPORTS and f"{name}(" in hdr and hasattr(L, name)
    assert "FPV_PHYS_ROWS" in hdr and "Per-drone physics" in hdr and "max_rates is\n * deliberately NOT per drone" in hdr
    assert L.fpv_abi_version() == 9 == _lib.FPV_ABI_VERSION
    assert L.fpv_sizeof(0) == C.sizeof(_lib.FpvParams) and L.fpv_sizeof(1) == C.sizeof(_lib.FpvBuffers)
    assert _lib.FpvBuffers.reset_pose.offset == C.sizeof(_lib.FpvBuffers) - 8 and _lib.FpvParams.reset_seed.offset == C.sizeof(_lib.FpvParams) - 8
    assert L.fpv_algorithmic_bytes(0) == 133
    # a null handle is refused; the shipped library has the kernels, so that is what it says
    assert L.fpv_set_physics(None, 4096, 64) == FPV_EINVAL and b"null handle" in L.fpv_last_error()


def test_fpv_hip_alone_builds_loads_and_says_what_it_lacks(tmp_path):
    """The sanitizer builds and the ISA tools compile fpv_hip.hip alone: it must link without the second unit, export every
    declared symbol, and refuse a physics table with a message that says why."""
    import torch  # noqa: F401  (the HIP runtime torch ships, as fpyv_amd._lib loads it)
    from __graft_entry__ import HIPCC_FLAGS, HIP_SRC
    out = str(tmp_path / "libfpv_alone.so")
    subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + HIPCC_FLAGS + ["-o", out, HIP_SRC], check=True, capture_output=True)
    A = C.CDLL(out, mode=C.RTLD_LOCAL)
    for name in _lib.EXPORTS:
        assert hasattr(A, name), name
    A.fpv_last_error.restype = C.c_char_p
    A.fpv_set_physics.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
    assert A.fpv_physics_rows() == 13
    assert A.fpv_set_physics(None, 4096, 64) == FPV_EINVAL
    assert b"not in this build" in A.fpv_last_error()
    assert A.fpv_set_physics(None, None, 0) == FPV_EINVAL and b"null handle" in A.fpv_last_error()        # unbinding needs no kernel
    # host arithmetic is in fpv_hip.hip / fpv_derive.h: the same table from either library
    cb = _lib.pack_params(_base())
    which, sets = dealt(parameter_sets(_base()), 16)
    rows = np.empty((13, 16), np.float32)
    A.fpv_physics_derive.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64]
    assert A.fpv_physics_derive(C.byref(cb), 16, sets.ctypes.data, rows.ctypes.data, 16) == 0
    assert np.array_equal(rows, physics.derive(cb, sets))
