"""The range sensor on the host (include/fpv_abi.h "Range scan") - no GPU needed: the kernel's lane function
(fpv_range_eval) on hand-made cases with exact answers and against a float64 NumPy restatement of the definition on a seeded
scene, fpv_rays_derive against NumPy, and the exports, sizes and refusals that need no device.

Measured on the seeded scene (1024 drones x 16 rays, CPU): 40.4 / 42.4 / 46.6 % of the pairs hit something with 1 / 4 / 8 objects,
0.59 / 2.54 % start inside an object with 4 / 8; the restatement's own margins leave out 0 / 0 / 0.006 % of the pairs; on every
pair kept hit, miss and the nearest object agree, and the worst range error is 23.4 fp32 ulps of max(range, distance to the
object's centre) - a shallow ray over the ground, where the fp32 rounding of d_z = (R d_b)_z is divided by d_z itself.  The bound
asserted is the next power of two at or above 4 x that: 128."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import range_scene as S
from conftest import REPO
from fpyv_amd import _lib
from fpyv_amd import rays as RY
from fpyv_amd.objects import Cylinder, Gate, Ground, Target, Trail

LEVEL = [1.0, 0.0, 0.0, 0.0]
ULP_BOUND = 128.0           # next power of two >= 4 x 23.4 (the worst error measured on the scene below; see the module docstring)


def _one(ray, p, objects, q=LEVEL, max_range=20.0):
    return RY.evaluate(RY.derive([ray]), max_range, [p], [q], objects)[0, 0]


# ---- T1: hand-made cases, each against the float written in the issue -----------------------------------------------------------
def test_ground_from_above_below_and_level():
    g = [Ground()]
    assert _one([0, 0, -1], [0, 0, 5], g) == np.float32(5.0)
    assert _one([0, 0, 1], [0, 0, 5], g) == np.float32(20.0)
    assert _one([1, 0, 0], [0, 0, 5], g) == np.float32(20.0)                # d_z == 0 over the ground
    down = RY.evaluate(RY.derive([[0, 0, -1], [0, 0, 1], [1, 0, 0], [0.3, -0.5, 0.2]]), 20.0, [[0, 0, -1]], [LEVEL], g)
    assert np.array_equal(down, np.zeros((4, 1), np.float32))               # below the ground: inside, 0 on every ray


def test_cylinder_wall_top_and_cap():
    cyl = [Cylinder([3.0, 0.0, 0.0], 1.0, 2.0)]
    assert _one([1, 0, 0], [0, 0, 1], cyl) == np.float32(2.0)
    assert _one([1, 0, 0], [0, 0, 2.5], cyl) == np.float32(20.0)            # passes over the top
    assert _one([0, 0, -1], [3, 0, 5], cyl) == np.float32(3.0)              # the cap, along the axis (d_x == d_y == 0)
    assert _one([0, 0, -1], [5, 0, 5], cyl) == np.float32(20.0)             # parallel to the axis, outside the wall: never
    assert _one([0, 0, 1], [3, 0.5, 1], cyl) == np.float32(0.0)             # inside


def test_sphere_hit_inside_yaw_empty_list_and_clip():
    sph = [Target([0.0, 4.0, 3.0], 1.0)]
    assert _one([0, 1, 0], [0, 0, 3], sph) == np.float32(3.0)
    assert _one([0, 1, 0], [0, 3.5, 3], sph) == np.float32(0.0)             # inside
    assert _one([0, 1, 0], [0, 0, 3], sph, max_range=2.5) == np.float32(2.5)    # max_range clips the 3.0
    assert _one([0, -1, 0], [0, 0, 3], sph) == np.float32(20.0)             # behind the drone
    # yawed 90 degrees about z, the body's +x ray points along world +y: it hits the sphere, the unyawed one does not
    c = np.sqrt(0.5)
    yawed = _one([1, 0, 0], [0, 0, 3], sph, q=[c, 0, 0, c])
    assert abs(yawed - 3.0) < 1e-5 and _one([1, 0, 0], [0, 0, 3], sph) == np.float32(20.0)
    assert np.array_equal(RY.evaluate(S.scene()[2], 20.0, [[0, 0, 5]], [LEVEL], []), np.full((16, 1), 20.0, np.float32))
    # gates and trails are not seen
    assert _one([1, 0, 0], [0, 0, 3], [Gate([2, 0, 3], np.eye(3), 1.0), Trail()]) == np.float32(20.0)


def test_parallel_and_degenerate_rays_give_no_nan():
    objs = S.world(8)
    axes = RY.derive([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [1, 1e-13, 0], [1e-13, 0, 1]])
    p = np.array([[0, 0, 5], [3, 0, 2], [3, 0, 9], [-6, 3, 0], [1.5, -6, 3], [0, 0, 0], [6, 6, 7], [-2, 2.5, -1]], np.float32)
    q = np.tile(np.array(LEVEL, np.float32), (len(p), 1))
    out = RY.evaluate(axes, 20.0, p, q, objs)
    assert np.isfinite(out).all() and (out >= 0).all() and (out <= 20).all()
    # a quaternion of zeros turns every ray into itself (R = I); nothing is NaN either
    assert np.isfinite(RY.evaluate(axes, 20.0, p, np.zeros_like(q), objs)).all()


# ---- T2: the float64 restatement on the seeded scene ------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [1, 4, 8])
def test_ranges_agree_with_the_float64_restatement(count):
    p, q, rays = S.scene()
    world = S.world(count)
    ref, which, keep, scale = S.restate(p, q, rays, world)
    got = RY.evaluate(rays, S.MAX_RANGE, p, q, world)
    assert got.shape == ref.shape == (16, 1024) and not np.isnan(got).any()
    # one object at a time: the list's range is the nearest of them, and says which object that is
    per = np.stack([RY.evaluate(rays, S.MAX_RANGE, p, q, [o]) for o in world])
    assert np.array_equal(per.min(0), got)
    nearest = np.where(got < S.MAX_RANGE, per.argmin(0), -1)
    left_out, hits, inside = (~keep).mean(), (ref < S.MAX_RANGE).mean(), (ref == 0.0).mean()
    err = np.abs(got.astype(np.float64) - ref) / np.spacing(scale.astype(np.float32)).astype(np.float64)
    print(f"{count} objects: left out {100 * left_out:.3f} %, hit {100 * hits:.1f} %, inside {100 * inside:.2f} %, "
          f"worst {err[keep].max():.1f} ulp (bound {ULP_BOUND:g})")
    assert left_out <= 0.01
    assert hits >= 0.30                                     # the scene cannot silently go empty
    if count == 8:
        assert inside >= 0.01
    assert np.array_equal(nearest[keep], which[keep])       # hit / miss / which object is nearest
    assert err[keep].max() <= ULP_BOUND


# ---- T3: fpv_rays_derive ----------------------------------------------------------------------------------------------------------
def test_rays_derive_is_the_double_normalisation_narrowed_once():
    rng = np.random.default_rng(3)
    d = rng.normal(size=(32, 3)) * np.exp(rng.uniform(-20, 20, (32, 1)))
    want = (d / np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])[:, None]).astype(np.float32)
    assert np.array_equal(RY.derive(d).view(np.uint32), want.view(np.uint32))
    for bad, k in (([[1, 0, 0], [0, 0, 0]], 1), ([[np.nan, 0, 1]], 0), ([[1, 0, 0], [0, 1, 0], [np.inf, 0, 0]], 2)):
        with pytest.raises(_lib.FpvError, match=f"ray {k}:"):
            RY.derive(bad)
    for count in (0, 33):
        with pytest.raises(_lib.FpvError, match="1..32"):
            RY.derive(np.ones((count, 3)))


def test_fan_and_grid():
    f = RY.fan(9, 120.0)
    assert f.shape == (9, 3) and np.allclose(f[4], [1, 0, 0]) and np.allclose(f[:, 2], 0)
    assert np.allclose(np.degrees(np.arctan2(f[:, 1], f[:, 0])), np.linspace(60, -60, 9), atol=1e-4)
    assert np.allclose(RY.fan(3, 90.0, pitch_deg=-30.0)[:, 2], -0.5, atol=1e-6) and np.allclose(RY.fan(1, 90.0), [[1, 0, 0]])
    g = RY.grid(8, 4, 90.0, 60.0)
    assert g.shape == (32, 3) and (g[:, 0] > 0).all() and np.allclose(np.linalg.norm(g, axis=1), 1, atol=1e-6)
    assert g[0, 1] > 0 and g[0, 2] > 0 and g[-1, 1] < 0 and g[-1, 2] < 0       # row-major from the top-left pixel
    assert np.allclose(g[:8, 1], -g[7::-1, 1], atol=1e-6)
    with pytest.raises(ValueError, match="32"):
        RY.grid(8, 5, 90.0, 60.0)
    with pytest.raises(ValueError, match="32"):
        RY.fan(33, 90.0)


# ---- T4: exports, sizes and the refusals that need no device --------------------------------------------------------------------
def _scan_struct(n=4, rays=None, max_range=20.0):
    s = _lib.pack_range_scan(RY.derive([[1, 0, 0], [0, 1, 0]]) if rays is None else rays, max_range)
    out = np.zeros((s.ray_count, n), np.float32)
    s.ranges, s.ranges_ld = out.ctypes.data, n
    return s, out


def test_exports_sizes_and_null_handle():
    L = _lib.lib()
    hdr = open(os.path.join(REPO, "include", "fpv_abi.h"), encoding="utf-8").read()
    for name in ("fpv_rays_derive", "fpv_range_scan", "fpv_range_eval"):
        assert name in _lib.EXPORTS and hasattr(L, name) and f"int {name}(" in hdr
    assert L.fpv_abi_version() == 9 and "#define FPV_ABI_VERSION 9" in hdr and "#define FPV_MAX_RAYS 32" in hdr
    assert L.fpv_sizeof(0) == C.sizeof(_lib.FpvParams) == 688 and L.fpv_sizeof(1) == C.sizeof(_lib.FpvBuffers) == 200
    assert L.fpv_sizeof(6) == C.sizeof(_lib.FpvRangeScan) == 424
    assert L.fpv_sizeof(9) < 0 and b"6 = fpv_range_scan_t" in L.fpv_last_error()
    s, _ = _scan_struct()
    b = _lib.FpvBuffers()
    assert L.fpv_range_scan(None, C.byref(b), C.byref(s), None) == -1 and b"null handle" in L.fpv_last_error()


def test_range_eval_checks_its_arguments():
    L = _lib.lib()
    p, q = np.zeros((4, 3), np.float32), np.tile(np.array(LEVEL, np.float32), (4, 1))
    call = lambda s, n=4: L.fpv_range_eval(C.byref(s), n, p.ctypes.data, q.ctypes.data)  # noqa: E731
    s, out = _scan_struct()
    assert call(s) == 0 and (out == 20.0).all()
    assert L.fpv_range_eval(None, 4, p.ctypes.data, q.ctypes.data) == -1 and b"null argument" in L.fpv_last_error()
    assert call(s, 0) == -1 and b"n must be positive" in L.fpv_last_error()
    for field, value, code, what in (("struct_size", 8, -1, b"struct_size"), ("ray_count", 0, -1, b"ray_count"), ("ray_count", 33, -1, b"ray_count"),
                                     ("max_range", 0.0, -1, b"max_range"), ("max_range", float("inf"), -1, b"max_range"),
                                     ("max_range", float("nan"), -1, b"max_range"), ("ranges", None, -1, b"ranges is null"),
                                     ("ranges_ld", 2, -4, b"ranges_ld"), ("ranges_ld", 6, -4, b"multiple of 4")):
        s, out = _scan_struct(n=8 if value == 6 else 4)
        setattr(s, field, value)
        assert call(s) == code and what in L.fpv_last_error(), (field, value, L.fpv_last_error())
    s, _ = _scan_struct()
    s.rays[1][0] = 0.5                                      # not a unit direction any more
    assert call(s) == -1 and b"ray 1 is not a unit direction" in L.fpv_last_error()
    objs = _lib.pack_objects([(0, 0, 0, 0, 0, 0)])
    for count, typ, what in ((9, 0, b"objects.count"), (-1, 0, b"objects.count"), (1, 3, b"unknown object type")):
        s, _ = _scan_struct()
        objs.count, objs.obj[0].type = count, typ
        s.objects = C.addressof(objs)
        assert call(s) == -1 and what in L.fpv_last_error()


def test_fpv_hip_alone_says_the_range_scan_is_not_in_this_build(tmp_path):
    """fpv_hip.hip alone still links, exports every name, answers "not in this build" for the launch, and derives and evaluates
    the same bits (the host arithmetic lives in fpv_hip.hip and its headers)."""
    import torch  # noqa: F401  (the HIP runtime torch ships, as fpyv_amd._lib loads it)
    from __graft_entry__ import HIPCC_FLAGS, HIP_SRC
    out = str(tmp_path / "libfpv_alone.so")
    subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + HIPCC_FLAGS + ["-o", out, HIP_SRC], check=True, capture_output=True)
    A = C.CDLL(out, mode=C.RTLD_LOCAL)
    for name in _lib.EXPORTS:
        assert hasattr(A, name), name
    A.fpv_last_error.restype = C.c_char_p
    A.fpv_range_scan.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    A.fpv_range_eval.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    A.fpv_rays_derive.argtypes = [C.c_int, C.c_void_p, C.c_void_p]
    s, _ = _scan_struct()
    b = _lib.FpvBuffers()
    assert A.fpv_range_scan(None, C.byref(b), C.byref(s), None) == -1 and b"not in this build" in A.fpv_last_error()
    d = np.random.default_rng(1).normal(size=(16, 3))
    rays = np.zeros((16, 3), np.float32)
    assert A.fpv_rays_derive(16, d.ctypes.data, rays.ctypes.data) == 0
    assert np.array_equal(rays.view(np.uint32), RY.derive(d).view(np.uint32))
    p, q, _ = S.scene()
    n = 256
    s = _lib.pack_range_scan(rays, S.MAX_RANGE)
    got = np.zeros((16, n), np.float32)
    objs = _lib.pack_objects([o.as_row() for o in S.world(8)])
    s.ranges, s.ranges_ld, s.objects = got.ctypes.data, n, C.addressof(objs)
    assert A.fpv_range_eval(C.byref(s), n, np.ascontiguousarray(p[:n]).ctypes.data, np.ascontiguousarray(q[:n]).ctypes.data) == 0
    assert np.array_equal(got.view(np.uint32), RY.evaluate(rays, S.MAX_RANGE, p[:n], q[:n], S.world(8)).view(np.uint32))
