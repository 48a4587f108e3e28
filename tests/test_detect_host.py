"""Object detections on the host (no GPU): the box table against the reference's own bbox3d, the lane function (fpv_detect_eval, the
kernel's arithmetic) against the g22 captures of the reference's bbox2d and pruning (tools/gen_detect_golden.py) through the guard
band of tests/detect_law.py, the options, the refusals, the binding and the build list.

Figures of the committed capture (seed 0): the largest |fp32 "float"-mode extreme - float64 extreme| is 1.652e-3 pixels, so the band
is 6.61e-3 pixels wide; it leaves out 0.55 % of the coordinates and none of the visible flags."""
import ctypes as C
import os

import numpy as np
import pytest

import detect_law
from conftest import REPO
from fpyv_amd import _lib
from fpyv_amd.camera import Camera, DepthCamera
from fpyv_amd.detect import BoxDetector
from fpyv_amd.objects import Cylinder, Gate, Ground, Target

LEVEL = np.array([[1.0, 0.0, 0.0, 0.0]])


@pytest.fixture(scope="module")
def cap():
    return detect_law.load()


@pytest.fixture(scope="module")
def world(cap):
    return detect_law.scene(cap)


@pytest.fixture(scope="module")
def results(cap, world):
    """evaluate() of both cameras in both pixel modes, once"""
    objs, gates = world
    return {(c, px): detect_law.detector(cap, c, px).evaluate(cap["p"], cap["q"], objs, gates) for c in range(2) for px in ("int", "float")}


# ---- the box table ------------------------------------------------------------------------------------------------------------
def test_the_box_table_matches_the_references_bbox3d(cap, world):
    objs, gates = world
    b = BoxDetector().boxes(objs, gates).astype(np.float64)
    ref = cap["bbox3d"]
    assert b.shape == (ref.shape[0], 6) == (12, 6)
    want = np.concatenate([ref.min(axis=1), ref.max(axis=1)], axis=1)
    # the reference's corner order: x from max for k >= 4, y for odd k, z for k in 2, 3, 6, 7
    for m in range(12):
        for k in range(8):
            assert np.array_equal(ref[m, k], [want[m, 3 * (k >> 2)], want[m, 1 + 3 * (k & 1)], want[m, 2 + 3 * ((k >> 1) & 1)]])
    spheres = [4, 5]                              # stand-ins in the capture: their box is this build's own definition
    keep = [m for m in range(12) if m not in spheres]
    ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    assert np.all(np.abs(b - want)[keep] <= 4 * ulp[keep]), np.abs(b - want)[keep].max()
    assert np.array_equal(b[spheres], want[spheres].astype(np.float32))                 # centre +- radius of float32 inputs: exact here or 1 ulp
    # the gates alone, and another resolution: a coarser outline is a smaller box for a round gate, the same for a rectangle
    g17, g5 = BoxDetector().boxes((), gates), BoxDetector(gate_resolution=5).boxes((), gates)
    assert np.array_equal(g17, b[6:].astype(np.float32))
    assert np.array_equal(g17[[0, 3]], g5[[0, 3]]) and np.all(g5[:, :3] >= g17[:, :3] - 1e-6) and np.all(g5[:, 3:] <= g17[:, 3:] + 1e-6)


def test_slot_order_skips_what_does_not_collide_and_follows_the_list(world):
    objs, gates = world
    mixed = [objs[1], gates[0], objs[0], objs[4]]
    b = BoxDetector().boxes(mixed, gates[:2])
    full = BoxDetector().boxes(objs, gates)
    assert np.array_equal(b, full[[1, 0, 4, 6, 7]])


# ---- the law ------------------------------------------------------------------------------------------------------------------
def test_the_band_is_what_this_capture_measures(cap):
    tol, coords, flags = detect_law.measure(cap)
    print(f"tol {tol:.4e} coordinates left out {coords:.4f} flags left out {flags:.4f}")
    assert 0.9 * detect_law.TOL <= tol <= detect_law.TOL                 # the literal is the measured value, rounded up
    assert coords <= 0.02 and flags <= 0.02


@pytest.mark.parametrize("pixels", ["int", "float"])
@pytest.mark.parametrize("c", [0, 1])
def test_evaluate_matches_the_capture_outside_the_guard_band(cap, results, c, pixels):
    n_c, out_c, n_v, out_v = detect_law.check_against_capture(cap, c, pixels, results[(c, pixels)])
    print(f"camera {c} {pixels}: {out_c} of {n_c} coordinates and {out_v} of {n_v} flags inside the band")
    assert out_c <= 0.02 * n_c and out_v <= 0.02 * n_v
    fr = cap["front"][c]
    assert (fr == 0).any() and ((fr > 0) & (fr < 8)).any() and (fr == 8).any()          # every kind of box is in the capture
    assert cap["kept"][c].any() and (~cap["kept"][c] & (fr > 0)).any()                   # seen, and in front but off the image


def test_int_mode_is_the_truncation_of_float_mode(results):
    for c in range(2):
        a, b = results[(c, "int")], results[(c, "float")]
        assert np.array_equal(a["boxes"], np.trunc(b["boxes"])) and np.array_equal(a["depth"], b["depth"])
        assert a["boxes"].dtype == np.float32 and a["visible"].dtype == bool


# ---- options ------------------------------------------------------------------------------------------------------------------
def test_clip_clamps_visible_boxes_and_leaves_the_others(cap, world, results):
    objs, gates = world
    for c, px in ((0, "int"), (0, "float"), (1, "int")):
        plain = results[(c, px)]
        got = detect_law.detector(cap, c, px, clip=True).evaluate(cap["p"], cap["q"], objs, gates)
        w, h = (float(x) for x in cap["cam_resolution"][c])
        want = plain["boxes"].copy()
        vis = plain["visible"]
        hi = np.array([w, h, w, h], dtype=np.float32)[None, :, None]
        want = np.where(vis[:, None, :], np.clip(want, 0.0, hi), want)
        assert vis.any() and (~vis).any() and np.any(want != plain["boxes"])
        assert np.array_equal(got["boxes"], want) and np.array_equal(got["visible"], vis) and np.array_equal(got["depth"], plain["depth"])


def test_the_own_target_slot_is_a_plain_slot_with_the_same_box(cap, world):
    objs, gates = world
    n = cap["p"].shape[0]
    rng = np.random.default_rng(3)
    centre = (cap["p"].T + rng.uniform(-6, 6, (3, n))).astype(np.float32)
    rad = rng.uniform(0.2, 1.0, n).astype(np.float32)
    det = detect_law.detector(cap, 0, "float")
    got = det.evaluate(cap["p"], cap["q"], objs, gates, target_rows=centre, target_radius=rad)
    one = det.evaluate(cap["p"], cap["q"], objs, gates, target_rows=centre, target_radius=0.5)
    assert got["boxes"].shape == (13, 4, n)
    base = det.evaluate(cap["p"], cap["q"], objs, gates)
    for k in ("boxes", "depth", "visible"):
        assert np.array_equal(got[k][:12], base[k])
    for i in range(n):
        for res, r in ((got, rad[i]), (one, np.float32(0.5))):
            box = np.concatenate([centre[:, i] - r, centre[:, i] + r]).astype(np.float32)
            alone = det.evaluate(cap["p"][i:i + 1], cap["q"][i:i + 1], boxes=box[None])
            for k in ("boxes", "depth", "visible"):
                assert np.array_equal(res[k][12, ..., i], alone[k][0, ..., 0]), (k, i)
    # the slot alone, without a table
    solo = det.evaluate(cap["p"], cap["q"], target_rows=centre, target_radius=rad)
    assert np.array_equal(solo["boxes"][0], got["boxes"][12]) and np.array_equal(solo["visible"][0], got["visible"][12])


def test_padded_rows_are_not_written(cap, world):
    objs, gates = world
    det = detect_law.detector(cap, 1)
    a = det.evaluate(cap["p"][:5], cap["q"][:5], objs, gates)
    b = det.evaluate(cap["p"][:5], cap["q"][:5], objs, gates, ld=16)
    for k in a:
        assert np.array_equal(a[k], b[k])
    L = _lib.lib()
    s, t = det.derive(), det.table(objs, gates)
    out, dep, vis = np.full((12, 4, 8), -7.0, np.float32), np.full((12, 8), -7.0, np.float32), np.full((12, 8), 9, np.uint8)
    s.table, s.boxes, s.box_depth, s.box_visible, s.ld = C.addressof(t), out.ctypes.data, dep.ctypes.data, vis.ctypes.data, 8
    t.count = 11
    p, q = np.ascontiguousarray(cap["p"][:5], np.float32), np.ascontiguousarray(cap["q"][:5], np.float32)
    assert L.fpv_detect_eval(C.byref(s), 5, p.ctypes.data, q.ctypes.data) == 0
    assert np.all(out[:, :, 5:] == -7.0) and np.all(dep[:, 5:] == -7.0) and np.all(vis[:, 5:] == 9)
    assert np.all(out[11] == -7.0) and np.all(vis[11] == 9) and np.array_equal(out[:11, :, :5], a["boxes"][:11])
    assert set(np.unique(vis[:11, :5])) <= {0, 1}


def test_a_box_behind_and_a_box_around_the_camera():
    det = BoxDetector(camera=Camera(0.0, [0.0, 0.0, 0.0], [640, 480], fov=90.0), pixels="float")
    p = [[0.0, 0.0, 5.0]]
    # the camera looks along the body x axis: a unit box 10 m ahead is centred on the image, 10 m behind it has no corner in front
    ahead = det.evaluate(p, LEVEL, boxes=[[9.5, -0.5, 4.5, 10.5, 0.5, 5.5]])
    assert ahead["visible"][0, 0] and np.allclose(ahead["depth"][0, 0], 9.5)
    assert np.allclose(ahead["boxes"][0, :, 0], [320 - 320 * 0.5 / 9.5, 240 - 320 * 0.5 / 9.5, 320 + 320 * 0.5 / 9.5, 240 + 320 * 0.5 / 9.5], atol=1e-3)
    behind = det.evaluate(p, LEVEL, boxes=[[-10.5, -0.5, 4.5, -9.5, 0.5, 5.5]])
    assert not behind["visible"][0, 0] and np.all(behind["boxes"] == 0.0) and behind["depth"][0, 0] == 0.0
    around = det.evaluate(p, LEVEL, boxes=[[-1.0, -1.0, 4.0, 1.0, 1.0, 6.0]])           # four corners in front at depth 1
    assert around["visible"][0, 0] and around["depth"][0, 0] == 1.0
    assert np.allclose(around["boxes"][0, :, 0], [0.0, -80.0, 640.0, 560.0])
    nan = det.evaluate([[np.nan, 0.0, 5.0]], LEVEL, boxes=[[9.5, -0.5, 4.5, 10.5, 0.5, 5.5]])
    assert not nan["visible"][0, 0]


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def test_every_refusal_names_its_reason(cap, world):
    objs, gates = world
    L = _lib.lib()
    det = BoxDetector()
    n = 3
    p, q = np.zeros((n, 3), np.float32), np.tile(LEVEL.astype(np.float32), (n, 1))
    out, dep, vis = np.zeros((13, 4, 4), np.float32), np.zeros((13, 4), np.float32), np.zeros((13, 4), np.uint8)
    rows = np.zeros((3, 4), np.float32)
    t = det.table(objs, gates)

    def good():
        s = det.derive()
        s.table, s.boxes, s.box_depth, s.box_visible, s.ld = C.addressof(t), out.ctypes.data, dep.ctypes.data, vis.ctypes.data, 4
        return s

    def refused(s, what, count=n, pp=p):
        rc = L.fpv_detect_eval(C.byref(s) if s is not None else None, count, pp.ctypes.data if pp is not None else None, q.ctypes.data)
        msg = L.fpv_last_error().decode()
        assert rc < 0 and what in msg, (rc, msg, what)

    assert L.fpv_detect_eval(C.byref(good()), n, p.ctypes.data, q.ctypes.data) == 0
    cases = [("struct_size", 0, "fpv_detect_t.struct_size"), ("width", 0, "width and height"), ("height", 20000, "width and height"),
             ("focal_length", float("nan"), "focal_length"), ("pixel_mode", 2, "unknown pixel mode"), ("boxes", None, "is null"),
             ("box_depth", None, "is null"), ("box_visible", None, "is null"), ("boxes", out.ctypes.data + 2, "4-byte aligned"),
             ("box_depth", dep.ctypes.data + 1, "4-byte aligned"), ("ld", 2, "ld is smaller"), ("ld", 6, "multiple of 4"), ("table", None, "1..72 boxes, not 0")]
    for field, value, what in cases:
        s = good()
        setattr(s, field, value)
        refused(s, what)
    s = good(); s.relative_rotation[4] = float("inf"); refused(s, "relative_rotation")
    s = good(); s.relative_position[1] = float("nan"); refused(s, "relative_position")
    s = good(); s.target_rows, s.target_ld = rows.ctypes.data, 2; refused(s, "target_ld")
    s = good(); s.target_rows, s.target_ld, s.target_radius_all = rows.ctypes.data, 4, -1.0; refused(s, "target_radius_all")
    for bad, what in ((np.nan, "box 2 is not finite"), (np.inf, "box 2 is not finite")):
        keep = t.box[2][4]
        t.box[2][4] = bad; refused(good(), what); t.box[2][4] = keep
    keep = t.box[5][0]
    t.box[5][0] = t.box[5][3] + 1.0; refused(good(), "box 5 has min > max"); t.box[5][0] = keep
    t.count = 73; refused(good(), "1..72 boxes, not 73"); t.count = -1; refused(good(), "1..72 boxes"); t.count = 12
    refused(None, "null argument"); refused(good(), "n must be positive", count=0); refused(good(), "null argument", pp=None)
    # through the Python class: 73 boxes, a NaN box, min > max, a bad ld
    one = [0.0, 0.0, 0.0, 1.0, 1.0, 1.0]
    with pytest.raises(_lib.FpvError, match="not 73"):
        det.evaluate(p, q, boxes=[one] * 73)
    with pytest.raises(_lib.FpvError, match="not 73"):
        det.evaluate(p, q, boxes=[one] * 72, target_rows=rows[:, :n])
    assert det.evaluate(p, q, boxes=[one] * 72)["boxes"].shape == (72, 4, n)
    with pytest.raises(_lib.FpvError, match="box 1 is not finite"):
        det.evaluate(p, q, boxes=[one, [0.0, np.nan, 0.0, 1.0, 1.0, 1.0]])
    with pytest.raises(_lib.FpvError, match="box 0 has min > max"):
        det.evaluate(p, q, boxes=[[0.0, 0.0, 2.0, 1.0, 1.0, 1.0]])
    with pytest.raises(_lib.FpvError, match="multiple of 4"):
        det.evaluate(p, q, boxes=[one], ld=6)
    with pytest.raises(_lib.FpvError, match="ld is smaller"):
        det.evaluate(p, q, boxes=[one], ld=0)
    # the table's own refusals name the slot
    with pytest.raises(_lib.FpvError, match="box 1: .*min > max"):
        det.boxes([Ground(60, 4), (1, 0.0, 0.0, 0.0, -1.0, 2.0)])
    with pytest.raises(_lib.FpvError, match="box 0: .*Ground"):
        det.boxes([Ground(-3.0, 4)])
    # a Ground that does not say how large it is has no box: the default Ground(), and a raw row
    with pytest.raises(_lib.FpvError, match="box 1: a Ground must be given its size"):
        det.boxes([Target([0, 0, 1], 1.0), Ground()])
    with pytest.raises(_lib.FpvError, match="box 0: a Ground must be given its size"):
        det.evaluate(p, q, [(0, 0.0, 0.0, 0.0, 0.0, 0.0)])
    with pytest.raises(_lib.FpvError, match="box 1: .*size of a gate"):
        det.boxes([Ground(60, 4)], [Gate(np.zeros(3), np.eye(3), 0.0)])
    with pytest.raises(ValueError, match="at most 8"):
        det.boxes([Target([0, 0, 1], 1.0)] * 9)
    with pytest.raises(ValueError, match="at most 64 gates"):
        det.boxes((), [Gate(np.zeros(3), np.eye(3), 1.0)] * 65)
    box = _lib.FpvBoxes()
    assert L.fpv_boxes_derive(None, None, None, 0, 0, C.byref(box)) < 0 and b"gate_resolution" in L.fpv_last_error()
    assert L.fpv_boxes_derive(None, None, None, 2, 17, C.byref(box)) < 0 and b"gates is null" in L.fpv_last_error()
    assert L.fpv_boxes_derive(None, None, None, 0, 17, None) < 0
    assert L.fpv_boxes_derive(None, None, None, 0, 17, C.byref(box)) == 0 and box.count == 0
    # unknown options: the reference's Gate raises NotImplementedError for a shape it does not know (components.py:802)
    with pytest.raises(ValueError, match="pixels must be"):
        BoxDetector(pixels="round")
    with pytest.raises(ValueError, match="gate_resolution"):
        BoxDetector(gate_resolution=0)
    with pytest.raises(NotImplementedError):
        det.boxes((), [Gate(np.zeros(3), np.eye(3), 1.0, shape="triangle")])


def test_derive_takes_the_references_camera_and_refuses_what_the_chase_refuses():
    L = _lib.lib()
    cam, out, ref = _lib.FpvCamera(), _lib.FpvDetect(), _lib.FpvChase()
    cam.pitch_deg, cam.fov_deg, cam.width, cam.height = 35.0, 120.0, 640, 480
    assert L.fpv_detect_derive(C.byref(cam), C.byref(out)) == 0 and L.fpv_chase_derive(C.byref(cam), C.byref(ref)) == 0
    assert out.focal_length == ref.focal_length and list(out.relative_rotation) == list(ref.relative_rotation) and (out.width, out.height) == (640, 480)
    cam.fov_deg = 180.0
    assert L.fpv_detect_derive(C.byref(cam), C.byref(out)) < 0 and b"fov" in L.fpv_last_error()
    assert L.fpv_detect_derive(None, C.byref(out)) < 0
    d = BoxDetector()                                           # None: the packaged parameters' camera, the reference's 640 x 480
    assert tuple(d.camera.resolution) == (640, 480) and d.derive().width == 640
    assert BoxDetector(camera=DepthCamera()).derive().width == 64


# ---- the C ABI and the build --------------------------------------------------------------------------------------------------
def test_struct_sizes_exports_and_the_build_list():
    L = _lib.lib()
    assert L.fpv_abi_version() == 9 == _lib.FPV_ABI_VERSION
    assert L.fpv_sizeof(0) == C.sizeof(_lib.FpvParams) == 688 and L.fpv_sizeof(1) == C.sizeof(_lib.FpvBuffers) == 200
    assert L.fpv_sizeof(2) == C.sizeof(_lib.FpvObjects) and _lib.FPV_MAX_OBJECTS == 8 and _lib.FPV_MAX_BOXES == 72
    assert L.fpv_sizeof(14) == C.sizeof(_lib.FpvDetect) and L.fpv_sizeof(16) == C.sizeof(_lib.FpvBoxes) == 4 + 72 * 24
    assert L.fpv_sizeof(13) < 0 and L.fpv_sizeof(15) < 0 and b"14 = fpv_detect_t, 16 = fpv_boxes_t" in L.fpv_last_error()
    import __graft_entry__ as entry
    assert entry.HIP_SRCS_DETECT == entry.HIP_SRCS_PNS + [os.path.join(REPO, "fpyv_amd", "csrc", "fpv_detect.hip")]
    new = ("fpv_boxes_derive", "fpv_detect_derive", "fpv_detect_boxes", "fpv_detect_eval")
    hdr = open(os.path.join(REPO, "include", "fpv_abi.h"), encoding="utf-8").read()
    for s in new:
        assert hasattr(L, s) and s in _lib.EXPORTS and f"int {s}(" in hdr, s
    assert "__global__" in open(os.path.join(REPO, "fpyv_amd", "csrc", "fpv_detect.hip"), encoding="utf-8").read()


def test_detecting_without_a_device_fails_loudly(cap, world):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    objs, gates = world
    L = _lib.lib()
    det = BoxDetector()
    t = det.table(objs, gates)
    out, dep, vis = np.zeros((12, 4, 4), np.float32), np.zeros((12, 4), np.float32), np.zeros((12, 4), np.uint8)
    s = det.derive()
    s.table, s.boxes, s.box_depth, s.box_visible, s.ld = C.addressof(t), out.ctypes.data, dep.ctypes.data, vis.ctypes.data, 4
    rc = L.fpv_detect_boxes(None, None, C.byref(s), None)
    assert rc == -3 and L.fpv_error_name(rc) == b"FPV_ENODEV" and b"HIP device" in L.fpv_last_error()
    s.ld = 6                                                     # the struct is checked first: no device needed to be told
    assert L.fpv_detect_boxes(None, None, C.byref(s), None) < 0 and b"multiple of 4" in L.fpv_last_error()
