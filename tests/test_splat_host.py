"""The point-cloud camera on the host (fpv_splat_eval, fpv_cloud_derive, fpyv_amd.clouds / splat) against g23_splat.npz, the capture
of the reference's own Camera.render_depth_image / render_image / pruned_objects_list and of its lit-pixel centroid
(tools/gen_splat_golden.py; 16 poses, none selected) - no GPU.  The images are held to the reference BYTE FOR BYTE, except on the
pixels the float64 capture alone marks fragile (tests/splat_law.py fragile): a point within TOL of a pixel boundary, a nearest depth
within TOL_B of a byte boundary (one level allowed).  TOL and TOL_B are 4 x the measured fp32 error, re-measured here."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import REPO, load_golden
import splat_law as L
from fpyv_amd import _lib
from fpyv_amd.clouds import PointCloud, cylinder_points, ground_points, icosphere
from fpyv_amd.objects import Cylinder, Gate, Ground, Target, Trail
from fpyv_amd.splat import PointCloudCamera


@pytest.fixture(scope="module")
def cap():
    return L.load()


@pytest.fixture(scope="module")
def rendered(cap):
    """the host images of both cameras, all encodings, once"""
    out = {}
    for c in range(2):
        for enc in ("u8", "mask", "metres"):
            out[c, enc] = L.camera(cap, c, encoding=enc).evaluate(cap["p"], cap["q"], L.cloud(cap))["image"]
    return out


def ulps_apart(got, want):
    """|got - want| in units of the fp32 spacing at `want`"""
    want32 = np.asarray(want, dtype=np.float32)
    return np.abs(np.asarray(got, dtype=np.float64) - np.asarray(want, dtype=np.float64)) / np.spacing(np.abs(want32)).astype(np.float64)


def test_derived_clouds_match_the_references_points_to_4_ulps(cap):
    cl = L.cloud(cap)
    assert cl.count == 12 and cl.total == int(cap["first"][-1]) == 2225 and np.array_equal(cl.first, cap["first"])
    for k in range(cl.count):
        want = cap["points"][cap["first"][k]:cap["first"][k + 1]]
        got = cl.world_points(k)
        assert got.shape == want.shape
        assert ulps_apart(got, want).max() <= 4.0, (k, ulps_apart(got, want).max())
        assert np.array_equal(cl.box[k, :3], cl.points[:, cl.first[k]:cl.first[k + 1]].min(axis=1))
        assert np.array_equal(cl.box[k, 3:], cl.points[:, cl.first[k]:cl.first[k + 1]].max(axis=1))
    # the boxes are helper_functions.bbox3d's: min and max of the points
    world_box = np.hstack([cl.box[:, :3] + cl.offset, cl.box[:, 3:] + cl.offset])
    want_box = np.hstack([cap["bbox3d"].min(axis=1), cap["bbox3d"].max(axis=1)])
    assert ulps_apart(world_box, want_box).max() <= 4.0
    assert np.all(cl.offset[cap["slot_kind"] != 2] == 0) and np.all(cl.offset[cap["slot_kind"] == 2] == cap["sph_position"].astype(np.float32))


def test_g19s_ground_and_cylinders_too():
    g = load_golden("g19_camera")
    size, res = g["ground_args"]
    assert ulps_apart(ground_points(size, int(res)), g["ground_points"]).max() <= 4.0
    for k in range(3):
        a = g["cylinder_args"][k]
        got = cylinder_points(a[:3], a[3], a[4], int(a[5]), int(a[6]))
        want = g[f"cylinder{k}_points"]
        assert got.shape == want.shape
        assert ulps_apart(got, want).max() <= 4.0


def test_the_capture_is_worth_comparing_with(cap):
    """from the float64 capture alone: lit share, every object kind lit, a pruned object, the column-0 quirk, few fragile pixels"""
    own = L.owner(cap)
    lit_total = pix_total = 0
    for c in range(2):
        img = cap[f"image{c}"]
        assert np.array_equal(L.image64(cap, c), img)                  # the float64 projection of the tests IS the reference's image
        lit_total += int((img > 0).sum()); pix_total += img.size
        hard, soft = L.fragile(cap, c)
        assert (hard | soft).mean() <= 0.02, (c, (hard | soft).mean())
        assert (~cap["kept"][c]).any() and cap["kept"][c].any()
    assert lit_total >= 0.05 * pix_total
    # each kind is the nearest point of a lit pixel in at least one pose (64 x 48)
    kinds = set()
    md = float(cap["max_depth"])
    for land in L.landing(cap, 0):
        zbuf = {}
        for j, x, y, z in zip(land["idx"], land["x"], land["y"], land["z"]):
            if (y, x) not in zbuf or z < zbuf[y, x][0]:
                zbuf[y, x] = (z, j)
        kinds |= {int(cap["slot_kind"][own[j]]) for z, j in zbuf.values() if int(255 * (1 - min(z, md) / md)) > 0}
    assert kinds == {0, 1, 2, 3}
    quirk = 0
    for c in range(2):
        for land in L.landing(cap, c):
            quirk += int(((land["u"] > -1) & (land["u"] < 0) & (land["x"] == 0)).sum())
    assert quirk > 0


def test_tol_and_tol_b_are_the_measured_ones(cap):
    rep = L.measure(cap)
    tol, tol_b = float(rep["tol (pixels)"]), float(rep["tol_b (levels)"])
    assert tol <= L.TOL <= 1.01 * tol and tol_b <= L.TOL_B <= 1.01 * tol_b, rep
    design = open(os.path.join(REPO, "DESIGN.md"), encoding="utf-8").read()
    assert f"{L.TOL:.2e}" in design and f"{L.TOL_B:.2e}" in design


def test_kept_flags_match_the_capture_outside_the_band(cap):
    cl = L.cloud(cap)
    for c in range(2):
        band = L.kept_band(cap, c)
        # the kept flag of an object is read off a render of that object alone
        for m in range(cl.count):
            one = PointCloud([cl.points[:, cl.first[m]:cl.first[m + 1]].T], [cl.offset[m]])
            got = L.camera(cap, c, encoding="mask").evaluate(cap["p"], cap["q"], one)["image"]
            lands = np.array([(np.isin(L.owner(cap)[ld["idx"]], [m])).any() for ld in L.landing(cap, c, kept=np.ones_like(cap["kept"][c]))])
            kept = cap["kept"][c][:, m]
            ok = ~band[:, m]
            # pruned: nothing of it may be drawn; kept and something lands in the image: it is drawn
            assert not got[ok & ~kept].any()
            assert got[ok & kept & lands].reshape(int((ok & kept & lands).sum()), -1).any(axis=1).all()


def test_images_equal_the_reference_byte_for_byte(cap, rendered):
    for c in range(2):
        hard, soft = L.fragile(cap, c)
        compared = L.compare(cap, c, rendered[c, "u8"], cap[f"image{c}"], hard, soft)
        assert compared >= 0.98 * hard.size
        # render_image: 1 where a point landed
        assert np.array_equal(rendered[c, "mask"][~hard], cap[f"mask{c}"][~hard])
        # metres: the depth the byte encodes; nothing landed: max_depth
        m = rendered[c, "metres"]
        assert m.dtype == np.float32 and np.all(m[rendered[c, "mask"] == 0] == np.float32(cap["max_depth"]))
        z = np.minimum(m, np.float32(cap["max_depth"]))
        assert np.array_equal((np.float32(255.0) * (np.float32(1.0) - z / np.float32(cap["max_depth"]))).astype(np.uint8), rendered[c, "u8"])


def test_centroid_of_the_target_only_image(cap):
    objs = L.scene(cap)
    md = float(cap["target_max_depth"])
    seen = unseen = 0
    for c in range(2):
        for k in range(2):
            t = objs[4 + k]
            got = L.camera(cap, c, max_depth=md, centroid=True).evaluate(cap["p"], cap["q"], [t])
            want_img = cap[f"target_image{c}"][:, k]
            hard, soft = L.fragile(cap, c, slots=[4 + k], max_depth=md)
            L.compare(cap, c, got["image"], want_img, hard, soft)
            same = (got["image"] == want_img).reshape(len(want_img), -1).all(axis=1)
            assert same.sum() >= len(same) - 1
            lit, cen = cap["target_lit"][c, :, k], cap["target_centroid"][c, :, k]
            assert np.array_equal(got["lit"][same], lit[same])
            some = same & (lit > 0)
            assert ulps_apart(got["centroid"][some], cen[some]).max() <= 1.0
            none = same & (lit == 0)
            assert np.isnan(got["centroid"][none]).all() and np.all(got["lit"][none] == 0)
            seen += int(some.sum()); unseen += int(none.sum())
    assert seen >= 8 and unseen >= 8


def test_a_moved_target_moves_only_the_offset(cap):
    t = Target([3.0, 0.0, 2.0], 0.5, 2, path=dict(radius=2.0, resolution=8))
    cl = PointCloud.from_world([Ground(20, 5), t, Trail()])
    assert cl.count == 2 and cl.total == 25 + 42
    before = cl.points.copy()
    cam = PointCloudCamera(resolution=(16, 12), centroid=True)
    p, q = [[0.0, 0.0, 2.0]], [[1.0, 0.0, 0.0, 0.0]]
    a = cam.evaluate(p, q, cl)
    t.update(); t.update()
    assert cl.refresh() and not cl.refresh()
    b = cam.evaluate(p, q, cl)
    assert np.array_equal(cl.points, before) and np.array_equal(cl.offset[1], t.position.astype(np.float32))
    fresh = cam.evaluate(p, q, PointCloud.from_world([Ground(20, 5), t]))
    assert np.array_equal(b["image"], fresh["image"]) and not np.array_equal(a["image"], b["image"])


def test_objects_keep_their_rendering_arguments():
    assert Ground(10, 3).points.shape == (9, 3) and Ground().points.shape == (0, 3)
    assert Cylinder([0, 0, 0], 1, 2, 5, 3).points.shape == (15, 3) and Cylinder([0, 0, 0], 1, 2).points.shape == (0, 3)
    assert Gate(np.zeros(3), np.eye(3), 2.0).points.shape == (5, 3) and Gate(np.zeros(3), np.eye(3), 2.0, "circle", 9).points.shape == (10, 3)
    assert Target([0, 0, 0], 2.0).points.shape == (12, 3) and Target([0, 0, 0], 2.0, 3).vertices.shape == (92, 3)
    assert np.allclose(np.linalg.norm(icosphere(3), axis=1), 1.0)
    assert np.allclose(Target([1, 2, 3], 2.0, vertices=[[0, 0, 1]]).points, [[1, 2, 5]])
    with pytest.raises(ValueError, match="random=True"):
        Ground(10, 3, random=True).points
    with pytest.raises(ValueError, match="random=True"):
        Cylinder([0, 0, 0], 1, 2, 5, 3, random=True).points

    class Raw:
        points = np.array([[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]])
    cl = PointCloud.from_world([Raw()], gates=[Gate(np.zeros(3), np.eye(3), 2.0)])
    assert cl.count == 2 and cl.first.tolist() == [0, 2, 7] and cl.point_ld == 8 and cl.box[0].tolist() == [1, 2, 3, 4, 5, 6]


def test_refusals_by_name():
    cam = PointCloudCamera(resolution=(16, 12), centroid=True)
    lib = _lib.lib()
    pts = np.zeros((3, 8), dtype=np.float32)
    img = np.zeros(16 * 12 + 4, dtype=np.uint8)
    cen, lit = np.zeros(2, dtype=np.float32), np.zeros(1, dtype=np.int32)
    p, q = np.zeros((1, 3), dtype=np.float32), np.array([[1, 0, 0, 0]], dtype=np.float32)

    def good():
        s = cam.derive()
        s.object_count = 2
        s.first[0], s.first[1], s.first[2] = 0, 3, 8
        for m in range(2):
            s.box[m][:] = [0, 0, 0, 1, 1, 1]
        s.points, s.point_ld, s.image, s.image_ld = pts.ctypes.data, 8, img.ctypes.data, 16 * 12
        s.centroid, s.lit = cen.ctypes.data, lit.ctypes.data
        return s

    def refused(match, code=None, n=1, **kw):
        s = good()
        for k, v in kw.items():
            setattr(s, k, v)
        with pytest.raises(_lib.FpvError, match=match):
            _lib.check(lib.fpv_splat_eval(C.byref(s), n, p.ctypes.data, q.ctypes.data))
        return s

    _lib.check(lib.fpv_splat_eval(C.byref(good()), 1, p.ctypes.data, q.ctypes.data))
    refused("struct_size", struct_size=8)
    refused("points is null", points=None)
    refused("points must be 4-byte aligned", points=pts.ctypes.data + 2)
    refused("image is null", image=None)
    refused("image must be 4-byte aligned", image=img.ctypes.data + 1)
    refused("image_ld is smaller", image_ld=16 * 12 - 4)
    refused("image_ld must be a multiple of 4", image_ld=16 * 12 + 2)
    refused("point_ld is smaller", point_ld=4)
    refused("point_ld must be a multiple of 4", point_ld=10)
    refused("centroid and lit", lit=None)
    refused("centroid and lit", centroid=None)
    refused("centroid and lit must be 4-byte aligned", centroid=cen.ctypes.data + 2)
    refused("width and height must be 4..128", width=132)
    refused("width and height must be 4..128", height=2)
    refused("width must be a multiple of 4", width=18)
    refused("focal_length", focal_length=0.0)
    refused("focal_length", focal_length=float("nan"))
    refused("unknown encoding", encoding=3)
    refused("max_depth", max_depth=0.0)
    refused("max_depth", max_depth=float("inf"))
    refused("object_count", object_count=73)
    refused("object_count", object_count=-1)
    refused("n must be positive", n=0)
    for setup, match in ((lambda s: s.first.__setitem__(0, 1), r"first\[0\]"), (lambda s: s.first.__setitem__(2, 2), "non-decreasing at object 1"),
                         (lambda s: s.first.__setitem__(2, (1 << 20) + 1), "past 2\\^20 points at object 1"),
                         (lambda s: s.box[1].__setitem__(4, float("nan")), "box 1 is not finite"),
                         (lambda s: s.box[0].__setitem__(0, 2.0), "box 0 has min > max"),
                         (lambda s: s.offset[1].__setitem__(2, float("inf")), "offset 1 is not finite"),
                         (lambda s: s.relative_rotation.__setitem__(4, float("nan")), "relative_rotation"),
                         (lambda s: s.relative_position.__setitem__(0, float("inf")), "relative_position")):
        s = good()
        setup(s)
        with pytest.raises(_lib.FpvError, match=match):
            _lib.check(lib.fpv_splat_eval(C.byref(s), 1, p.ctypes.data, q.ctypes.data))
    # the struct is checked before the handle: a null handle meets the struct's refusal first, then - here, without a device - ENODEV
    s = good()
    s.encoding = 7
    with pytest.raises(_lib.FpvError, match="unknown encoding"):
        _lib.check(lib.fpv_splat_render(None, None, C.byref(s), None))
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(_lib.FpvError, match="no HIP device"):
            _lib.check(lib.fpv_splat_render(None, None, C.byref(good()), None))
    with pytest.raises(_lib.FpvError, match="4..128"):
        PointCloudCamera(resolution=(640, 480)).derive()
    with pytest.raises(ValueError, match="encoding"):
        PointCloudCamera(encoding="rgb")
    with pytest.raises(ValueError, match="at most 72 objects"):
        PointCloud([np.zeros((1, 3))] * 73)
    assert lib.fpv_sizeof(18) == C.sizeof(_lib.FpvSplat) and lib.fpv_sizeof(17) < 0 and lib.fpv_abi_version() == 9
    num, res = (C.c_double * 1)(10.0), (C.c_int32 * 1)(0)
    assert lib.fpv_cloud_derive(0, C.addressof(num), C.addressof(res), None, 0) < 0 and "resolution" in _lib.lib().fpv_last_error().decode()
    res[0] = 2000
    assert lib.fpv_cloud_derive(0, C.addressof(num), C.addressof(res), None, 0) < 0 and "2^20" in _lib.lib().fpv_last_error().decode()
    assert lib.fpv_cloud_derive(5, C.addressof(num), C.addressof(res), None, 0) < 0


def test_degenerate_worlds():
    cam = PointCloudCamera(resolution=(8, 4), max_depth=10.0, centroid=True)
    p, q = [[0.0, 0.0, 1.0]], [[1.0, 0.0, 0.0, 0.0]]
    empty = cam.evaluate(p, q, PointCloud([]))
    assert np.all(empty["image"] == 0) and empty["lit"][0] == 0 and np.isnan(empty["centroid"]).all()
    nopoints = cam.evaluate(p, q, PointCloud([np.zeros((0, 3)), np.zeros((0, 3))]))
    assert np.all(nopoints["image"] == 0)
    m = PointCloudCamera(resolution=(8, 4), max_depth=10.0, encoding="metres").evaluate(p, q, PointCloud([]))["image"]
    assert np.all(m == np.float32(10.0))
