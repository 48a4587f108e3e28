"""The depth camera on the host (include/fpv_abi.h "Depth camera") - no GPU needed: fpv_camera_derive and a float64
restatement of the definition against the reference's own Camera numbers and point clouds (tests/golden/g19_camera.npz), the
kernel's pixel function (fpv_depth_eval) against the restatement on a seeded scene, the byte encoding, edge cases, and the
exports, sizes and refusals that need no device.

Measured on the seeded scene (256 drones, 32 x 24 pixels, max_depth 25; CPU) - objects / gates: share of pixels that hit something,
share that hit a gate frame, share of pixel-thing pairs the restatement's margins leave out, worst depth error in fp32 ulps of
max(depth, distance to the thing's centre):
    0 / 1     hit  0.2 %   frame  0.17 %   left out 0.0036 %   worst  17.8 ulp
    4 / 12    hit 22.0 %   frame  2.58 %   left out 0.0037 %   worst  53.2 ulp
    8 / 64    hit 32.3 %   frame  9.89 %   left out 0.0042 %   worst  73.7 ulp
    8 / 0     hit 25.2 %   frame  0    %   left out 0.0013 %   worst 127.997 ulp
    0 / 64    hit 11.4 %   frame 11.40 %   left out 0.0046 %   worst  73.7 ulp
    4 / 1     hit 20.1 %   frame  0.16 %   left out 0.0014 %   worst  41.4 ulp
    0 / 12    hit  2.7 %   frame  2.69 %   left out 0.0046 %   worst  53.2 ulp
On every pixel kept hit, miss and the nearest thing agree.  The worst error, 127.997 ulp, is a ray that grazes the ball of a Target
2 m away (discriminant 1.3e-4 of r^2, just above the 1e-4 margin): the half chord is the root of a difference that has lost
four digits.  The worst on a gate, 73.7 ulp, is a plane met at a shallow angle: t = -s / (n.d) divides by an n.d of which the fp32
rounding of d = R d_b is a larger share the flatter the ray runs.  The restatement forms its directions from the reference's
float64 camera formulas, not from the narrowed vectors of fpv_camera_derive: their rounding is part of what is measured.  The
bound asserted is the next power of two at or above 4 x the worst (511.99): 512.  The byte encoding: 99.9995 % of the bytes equal the
reference's float64 formula applied to the fp32 depth, the rest differ by one level."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import depth_scene as S
from conftest import REPO
from fpyv_amd import _lib
from fpyv_amd import gates as GT
from fpyv_amd.camera import Camera, DepthCamera
from fpyv_amd.objects import Cylinder, Gate, Ground, Target

LEVEL = [1.0, 0.0, 0.0, 0.0]
ULP_BOUND = 512.0           # next power of two >= 4 x the worst error measured on the scene below (see the module docstring)
GOLD = os.path.join(REPO, "tests", "golden", "g19_camera.npz")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


# ---- (a) the derive and the restatement against the reference's camera ----------------------------------------------------------
def test_camera_numbers_are_the_references(gold):
    W, H = (int(x) for x in gold["resolution"])
    cam = Camera(float(gold["camera_pitch_angle"]), gold["position_relative_to_frame"], [W, H], fov=float(gold["fov"]))
    s = cam.derive()
    # the derive: focal length and relative rotation in double, the narrowed direction vectors to fp32 rounding
    assert abs(cam.focal_length - float(gold["focal_length"])) <= 1e-12
    assert np.abs(cam.relative_rotation_matrix - gold["relative_rotation_matrix"]).max() <= 1e-12
    assert np.abs(cam.intrinsic_matrix - gold["intrinsic_matrix"]).max() <= 1e-12
    f, rr = float(gold["focal_length"]), gold["relative_rotation_matrix"]
    a0 = rr @ np.array([(0.5 - W / 2) / f, (0.5 - H / 2) / f, 1.0])
    for got, want in ((s.dir0, a0), (s.dir_u, rr[:, 0] / f), (s.dir_v, rr[:, 1] / f), (s.offset, gold["position_relative_to_frame"])):
        assert np.array_equal(np.array(got[:], np.float32), want.astype(np.float32))
    corner = np.sqrt(1 + (W / 2 / f) ** 2 + (H / 2 / f) ** 2)
    assert corner <= s.dir_len_max <= corner * (1 + 1e-6)
    # the restatement: focal length, origin, camera rotation, and every recorded direction = the normalised C d_c
    assert abs(S.focal(W, float(gold["fov"])) - f) <= 1e-12 and np.abs(S.rel_rot(float(gold["camera_pitch_angle"])) - rr).max() <= 1e-12
    Kinv = np.linalg.inv(gold["intrinsic_matrix"])
    for k in range(len(gold["drone_position"])):
        R = gold["drone_rotation_matrix"][k]
        o = gold["drone_position"][k] + R @ gold["position_relative_to_frame"]
        Cm = R @ S.rel_rot(float(gold["camera_pitch_angle"]))
        assert np.abs(o - gold["position"][k]).max() <= 1e-12 and np.abs(Cm - gold["rotation_matrix"][k]).max() <= 1e-12
        # the derive's rotation on the same pose
        assert np.abs(R @ cam.relative_rotation_matrix - gold["rotation_matrix"][k]).max() <= 1e-12
        for px, dd, dw in zip(gold["pixels"], gold["direction_drone"][k], gold["direction_world"][k]):
            dc = Kinv @ np.array([px[0], px[1], 1.0])
            assert np.abs(S.rel_rot(35.0) @ dc / np.linalg.norm(dc) - dd).max() <= 1e-12
            assert np.abs(Cm @ dc / np.linalg.norm(dc) - dw).max() <= 1e-12
            # ... and the derive's affine form of it, in double from the double rotation
            i, j = px[0] - 0.5, px[1] - 0.5
            db = a0 + i * rr[:, 0] / f + j * rr[:, 1] / f
            assert np.abs(db / np.linalg.norm(db) - dd).max() <= 1e-12
    # the pixel centres of the restatement are K^-1 (i + 1/2, j + 1/2, 1)
    dirs = S.pixel_dirs_cam(W, H, float(gold["fov"]))
    assert np.abs(dirs[5, 7] - Kinv @ np.array([7.5, 5.5, 1.0])).max() <= 1e-12 and (dirs[..., 2] == 1.0).all()


# ---- (b) the restatement against the reference's point clouds --------------------------------------------------------------------
def test_restatement_sees_the_references_clouds_at_their_depth(gold):
    world = [Ground()] + [Cylinder(list(c[:3]), float(c[3]), float(c[4])) for c in gold["cylinder_args"]]
    clouds = [("ground", gold["ground_points"], None)] + [(f"cylinder {k}", gold[f"cylinder{k}_points"], gold["cylinder_args"][k])
                                                           for k in range(len(gold["cylinder_args"]))]
    for name, pts, args in clouds:
        kept = below = equal = 0
        worst = 0.0
        for k in range(len(gold["position"])):
            o, Cm = gold["position"][k], gold["rotation_matrix"][k]
            pc = (pts - o) @ Cm                              # camera frame: rows of C^T (x - o)
            z = pc[:, 2]
            ok = z > 0.1
            if args is not None:                             # the rim rows sit on the slab boundary and round either way
                ok &= (np.abs(pts[:, 2] - args[2]) > 1e-6) & (np.abs(pts[:, 2] - (args[2] + args[4])) > 1e-6)
            # the reference's depth is the third row of projection_matrix @ point
            zr = (gold["projection_matrix"][k] @ np.vstack([pts.T, np.ones(len(pts))]))[2]
            assert np.abs(zr - z).max() <= 1e-9
            if not ok.any():                                 # wholly behind this pose's camera
                continue
            d = (pc[ok] / z[ok, None]) @ Cm.T                # the ray to the point: camera-frame z = 1
            depth, _, _, _, _ = S.cast(np.repeat(o[None], ok.sum(), 0).astype(np.float64), d, world, max_depth=1e9)
            kept += int(ok.sum())
            below += int((depth <= z[ok] * (1 + 1e-9) + 1e-9).sum())
            worst = max(worst, float(((depth - z[ok]) / z[ok]).max()))
            equal += int((np.abs(depth - z[ok]) <= 1e-9).sum())
        print(f"{name}: kept {kept}, depth <= z on {below}, worst excess {worst:.1e} (relative), depth = z on {equal / kept:.2f}")
        assert kept > 300 and below == kept
        assert equal / kept >= 0.25


# ---- (c) the fp32 pixel function against the restatement --------------------------------------------------------------------------
CASES = [(0, 1), (4, 12), (8, 64), (8, 0), (0, 64), (4, 1), (0, 12)]


@pytest.fixture(scope="module")
def seeded():
    cam = DepthCamera(resolution=(32, 24), max_depth=S.MAX_DEPTH)
    p, q = S.scene()
    return cam, p, q


@pytest.mark.parametrize("objects,gates", CASES)
def test_images_agree_with_the_float64_restatement(seeded, objects, gates):
    cam, p, q = seeded
    world = S.world(objects)
    rows = GT.derive(S.course(gates)) if gates else None
    ref, which, keep, scale, (pairs, dropped) = S.restate(p, q, cam, world, rows)
    got = cam.evaluate(p, q, world, rows)
    assert got.shape == ref.shape == (256, 24, 32) and got.dtype == np.float32 and not np.isnan(got).any()
    # one thing at a time: the image is the nearest of them, and says which thing that is
    per = [cam.evaluate(p, q, [o]) for o in world] + [cam.evaluate(p, q, (), rows[g:g + 1]) for g in range(gates)]
    ids = np.array(list(range(objects)) + [100 + g for g in range(gates)])
    per = np.stack(per)
    assert np.array_equal(per.min(0), got)
    nearest = np.where(got < cam.max_depth, ids[per.argmin(0)], -1)
    if gates >= 3:                                           # all three shapes: r2 = inf the rectangle, zc != 0 the half circle
        assert {bool(np.isinf(r[15])) for r in rows} == {True, False} and any(r[14] != 0 for r in rows)
    left_out, hits, frames = dropped / max(pairs, 1), (ref < cam.max_depth).mean(), (which >= 100).mean()
    err = np.abs(got.astype(np.float64) - ref) / np.spacing(scale.astype(np.float32)).astype(np.float64)
    at = np.unravel_index(np.argmax(np.where(keep, err, 0.0)), err.shape)
    print(f"{objects} objects / {gates} gates: hit {100 * hits:.1f} %, gate frame {100 * frames:.2f} %, left out {100 * left_out:.4f} % "
          f"of {pairs} pairs, worst {err[keep].max():.1f} ulp at {at} (thing {which[at]}, depth {ref[at]:.3f}; bound {ULP_BOUND:g})")
    assert left_out <= 0.01
    # the floors of the scene (it cannot silently go empty) hold where they can: a case without objects sees no ground and one
    # with a single gate next to no frame (0 / 1 hits 0.2 % of the pixels), so they are asserted for the two cases that have both
    if (objects, gates) in ((4, 12), (8, 64)):
        assert hits >= 0.20 and frames >= 0.02
    assert np.array_equal(nearest[keep], which[keep])        # hit / miss / which thing is nearest
    assert err[keep].max() <= ULP_BOUND


# ---- (d) the byte encoding -----------------------------------------------------------------------------------------------------------
def test_u8_is_the_references_byte_of_the_fp32_depth(seeded):
    cam, p, q = seeded
    world, rows = S.world(8), GT.derive(S.course(12))
    metres = cam.evaluate(p, q, world, rows)
    u8 = DepthCamera(resolution=(32, 24), max_depth=S.MAX_DEPTH, encoding="u8").evaluate(p, q, world, rows)
    assert u8.dtype == np.uint8 and u8.shape == metres.shape
    want = (255 * (1 - metres.astype(np.float64) / S.MAX_DEPTH)).astype(np.uint8)       # components.py:628 on the fp32 depth
    diff = np.abs(u8.astype(np.int32) - want.astype(np.int32))
    print(f"u8: {100 * (diff == 0).mean():.4f} % of {diff.size} bytes equal the float64 formula's, the rest differ by {diff.max()}")
    assert diff.max() <= 1
    assert u8[metres == S.MAX_DEPTH].max() == 0 and (u8[metres == 0.0] == 255).all()
    # the written-down fp32 form, exactly
    q32 = metres / np.float32(S.MAX_DEPTH)
    assert np.array_equal(u8, (np.float32(255.0) * (np.float32(1.0) - q32)).astype(np.uint8))


# ---- (e) edge cases --------------------------------------------------------------------------------------------------------------
def test_hand_made_views():
    cam = DepthCamera(resolution=(8, 8), fov=90.0, camera_angle=0.0, position_relative_to_frame=(0, 0, 0), max_depth=20.0)
    # level, 5 m up: the rows below the horizon see the ground at z-depth 5 / tan(angle below), the rows above see nothing
    img = cam.evaluate([[0, 0, 5]], [LEVEL], [Ground()])[0]
    f = 4.0
    for j in range(8):
        down = (j + 0.5 - 4.0) / f                           # image rows run downwards: body z = -y_c
        want = 5.0 / down if down > 0 and 5.0 / down < 20 else 20.0
        assert np.allclose(img[j], want, rtol=1e-6), (j, img[j], want)
    # a gate straight ahead at x = 4 (pixel centres there are 1 m apart: +-0.5, +-1.5 ...): the aperture |y|, |z| <= 1 shows what
    # is behind it, the frame out to 1.75 is at depth 4 - the ring of twelve pixels around the middle four
    wide = DepthCamera(resolution=(8, 8), fov=90.0, camera_angle=0.0, position_relative_to_frame=(0, 0, 0), max_depth=20.0,
                       gate_frame=0.75)
    gate = [Gate([4.0, 0.0, 5.0], np.eye(3), 2.0)]
    front = wide.evaluate([[0, 0, 5]], [LEVEL], [], gate)[0]
    ring = np.zeros((8, 8), bool)
    ring[2:6, 2:6] = True
    ring[3:5, 3:5] = False
    assert np.array_equal(front == 4.0, ring) and (front[~ring] == 20.0).all()
    back = wide.evaluate([[8, 0, 5]], [[0, 0, 0, 1]], [], gate)[0]          # from behind, yawed by 180 degrees: both faces are seen
    assert np.array_equal(back, front)
    assert (wide.evaluate([[0, 0, 5]], [LEVEL], [], [Gate([30.0, 0.0, 5.0], np.eye(3), 2.0)]) == 20.0).all()   # beyond max_depth
    # inside a solid: 0 on every pixel
    assert (cam.evaluate([[0, 0, 3]], [LEVEL], [Target([0, 0, 3], 1.0)]) == 0.0).all()
    assert (cam.evaluate([[0, 0, -1]], [LEVEL], [Ground()]) == 0.0).all()


def test_parallel_and_degenerate_rays_give_no_nan():
    # an even image height and no pitch: no pixel has d_z == 0, so pitch the camera until a row's centre is level
    cam = DepthCamera(resolution=(8, 8), fov=90.0, camera_angle=float(np.rad2deg(np.arctan(0.125))), position_relative_to_frame=(0, 0, 0),
                      max_depth=20.0)
    zero = DepthCamera(resolution=(8, 8), fov=90.0, camera_angle=0.0, position_relative_to_frame=(0, 0, 0), max_depth=20.0)
    objs = S.world(8)
    gates = S.course(12) + [Gate([0.0, 0.0, 5.0], np.array([[0.0, 0, 1], [0, 1, 0], [-1, 0, 0]]), 2.0)]   # its plane z = 5 holds a drone
    p = np.array([[0, 0, 5], [3, 0, 2], [3, 0, 9], [-6, 3, 0], [1.5, -6, 3], [0, 0, 0], [9, 0, 3], [-2, 2.5, -1]], np.float32)
    q = np.tile(np.array(LEVEL, np.float32), (len(p), 1))
    for c in (cam, zero):
        for qq in (q, np.zeros_like(q)):                     # a quaternion of zeros: R = I
            out = c.evaluate(p, qq, objs, gates)
            assert np.isfinite(out).all() and (out >= 0).all() and (out <= 20).all()
    # d_z == 0 exactly (body x ahead, level) over the ground: max_depth above it, 0 below
    s = zero.derive()
    s.dir0[:], s.dir_u[:], s.dir_v[:] = [1.0, 0.0, 0.0], [0.0, 0.01, 0.0], [0.0, 0.0, 0.0]
    out = np.zeros((2, 8, 8), np.float32)
    objs1 = _lib.pack_objects([Ground().as_row()])
    s.image, s.image_stride, s.objects = out.ctypes.data, 64, C.addressof(objs1)
    pp, q2 = np.array([[0, 0, 5], [0, 0, -1]], np.float32), np.tile(np.array(LEVEL, np.float32), (2, 1))
    assert _lib.lib().fpv_depth_eval(C.byref(s), 2, pp.ctypes.data, q2.ctypes.data) == 0
    assert (out[0] == 20.0).all() and (out[1] == 0.0).all()


# ---- exports, sizes and the refusals that need no device --------------------------------------------------------------------------
def _render_struct(n=2, cam=None):
    cam = cam or DepthCamera(resolution=(8, 4))
    s = cam.derive()
    out = np.zeros((n, 4, 8), cam.dtype)
    s.image, s.image_stride = out.ctypes.data, 32
    return s, out


def test_exports_sizes_and_null_handle():
    L = _lib.lib()
    hdr = open(os.path.join(REPO, "include", "fpv_abi.h"), encoding="utf-8").read()
    for name in ("fpv_camera_derive", "fpv_depth_render", "fpv_depth_eval"):
        assert name in _lib.EXPORTS and hasattr(L, name) and f"int {name}(" in hdr
    assert L.fpv_abi_version() == 9 and "#define FPV_ABI_VERSION 9" in hdr
    assert L.fpv_sizeof(0) == C.sizeof(_lib.FpvParams) == 688 and L.fpv_sizeof(1) == C.sizeof(_lib.FpvBuffers) == 200
    assert L.fpv_sizeof(7) == C.sizeof(_lib.FpvDepthRender) == 192
    assert L.fpv_sizeof(9) < 0 and b"7 = fpv_depth_render_t" in L.fpv_last_error()
    s, _ = _render_struct()
    b = _lib.FpvBuffers()
    assert L.fpv_depth_render(None, C.byref(b), C.byref(s), None) == -1 and b"null handle" in L.fpv_last_error()


def test_camera_derive_names_what_it_refuses():
    for kw, what in ((dict(resolution=(2, 8)), "4..128"), (dict(resolution=(8, 132)), "4..128"), (dict(resolution=(10, 8)), "multiple of 4"),
                     (dict(fov=180.0), "fov"), (dict(fov=float("nan")), "fov"), (dict(camera_angle=float("inf")), "pitch"),
                     (dict(position_relative_to_frame=(0, float("nan"), 0)), "relative position")):
        with pytest.raises(_lib.FpvError, match=what):
            DepthCamera(**kw).derive()
    with pytest.raises(ValueError, match="encoding"):
        DepthCamera(encoding="half")
    assert DepthCamera.from_params({"camera": {"camera_angle": 35.0, "position_relative_to_frame": [0.1, 0, 0], "fov": 120.0,
                                               "resolution": [640, 480]}}, resolution=(64, 48)).resolution == (64, 48)


def test_depth_eval_checks_its_arguments():
    L = _lib.lib()
    p, q = np.zeros((2, 3), np.float32), np.tile(np.array(LEVEL, np.float32), (2, 1))
    call = lambda s, n=2: L.fpv_depth_eval(C.byref(s), n, p.ctypes.data, q.ctypes.data)  # noqa: E731
    s, out = _render_struct()
    assert call(s) == 0 and (out == 25.0).all()
    assert L.fpv_depth_eval(None, 2, p.ctypes.data, q.ctypes.data) == -1 and b"null argument" in L.fpv_last_error()
    assert call(s, 0) == -1 and b"n must be positive" in L.fpv_last_error()
    rows = np.zeros((1, 16), np.float32)
    for field, value, code, what in (("struct_size", 8, -1, b"struct_size"), ("width", 0, -1, b"4..128"), ("height", 129, -1, b"4..128"),
                                     ("width", 6, -1, b"multiple of 4"), ("encoding", 2, -1, b"encoding"),
                                     ("max_depth", 0.0, -1, b"max_depth"), ("max_depth", float("inf"), -1, b"max_depth"),
                                     ("max_depth", float("nan"), -1, b"max_depth"), ("image", None, -1, b"image is null"),
                                     ("image_stride", 28, -4, b"image_stride"), ("image_stride", 34, -4, b"multiple of 4"),
                                     ("gate_count", -1, -1, b"gate_count"), ("gate_count", 65, -1, b"gate_count"),
                                     ("gate_count", 1, -1, b"gates without descriptors"), ("dir_len_max", 0.5, -1, b"dir_len_max")):
        s, out = _render_struct()
        setattr(s, field, value)
        assert call(s) == code and what in L.fpv_last_error(), (field, value, L.fpv_last_error())
    for fw in (0.0, float("nan"), float("inf")):
        s, out = _render_struct()
        s.gate_count, s.gate_descriptors, s.gate_frame_width = 1, rows.ctypes.data, fw
        assert call(s) == -1 and b"gate_frame_width" in L.fpv_last_error()
    objs = _lib.pack_objects([(0, 0, 0, 0, 0, 0)])
    for count, typ, what in ((9, 0, b"objects.count"), (-1, 0, b"objects.count"), (1, 3, b"unknown object type")):
        s, _ = _render_struct()
        objs.count, objs.obj[0].type = count, typ
        s.objects = C.addressof(objs)
        assert call(s) == -1 and what in L.fpv_last_error()
    # a stride larger than the image leaves its padding alone
    s, _ = _render_struct()
    big = np.full((2, 40), -1.0, np.float32)
    s.image, s.image_stride = big.ctypes.data, 40
    assert call(s) == 0 and (big[:, :32] == 25.0).all() and (big[:, 32:] == -1.0).all()


def test_fpv_hip_alone_says_the_depth_camera_is_not_in_this_build(tmp_path):
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
    A.fpv_depth_render.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    A.fpv_depth_eval.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    A.fpv_camera_derive.argtypes = [C.c_void_p, C.c_void_p]
    s, _ = _render_struct()
    b = _lib.FpvBuffers()
    assert A.fpv_depth_render(None, C.byref(b), C.byref(s), None) == -1 and b"not in this build" in A.fpv_last_error()
    cam = DepthCamera(resolution=(32, 24))
    mine = cam.derive()
    c = _lib.FpvCamera()
    c.pitch_deg, c.fov_deg, c.width, c.height = cam.camera_angle, cam.fov, 32, 24
    c.relative_position[:] = list(cam.relative_position)
    theirs = _lib.FpvDepthRender.from_buffer_copy(mine)
    theirs.dir0[:] = [0.0, 0.0, 0.0]
    assert A.fpv_camera_derive(C.byref(c), C.byref(theirs)) == 0 and bytes(theirs) == bytes(mine)
    p, q = S.scene()
    n = 32
    rows = np.ascontiguousarray(GT.derive(S.course(12)))
    from fpyv_amd.camera import gate_rows
    rows = gate_rows(rows)
    got = np.zeros((n, 24, 32), np.float32)
    objs = _lib.pack_objects([o.as_row() for o in S.world(8)])
    theirs.image, theirs.image_stride, theirs.objects = got.ctypes.data, 768, C.addressof(objs)
    theirs.gate_descriptors, theirs.gate_count = rows.ctypes.data, 12
    assert A.fpv_depth_eval(C.byref(theirs), n, np.ascontiguousarray(p[:n]).ctypes.data, np.ascontiguousarray(q[:n]).ctypes.data) == 0
    assert np.array_equal(got.view(np.uint32), cam.evaluate(p[:n], q[:n], S.world(8), rows).view(np.uint32))
