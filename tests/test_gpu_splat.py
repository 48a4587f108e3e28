"""The point-cloud camera on the GPU (include/fpv_abi.h "Point-cloud camera"): the kernel against PointCloudCamera.evaluate -
its own point and pixel functions on the host - BIT FOR BIT, images, centroid and lit alike, on the poses read back from the batch,
with guard words behind every image, behind centroid and lit and NaN in the points' padding; object sizes around the workgroup's
stride; worlds that are pruned away or behind the camera; many points in one pixel; the column-0 quirk; a moved Target, moved
gates; the g23 capture of the reference on the device; FpvVecEnv(cloud_camera=) with partitions and auto-resets; poses no flight
visits."""
import functools

import numpy as np
import pytest
import torch

import splat_law as L
from fpyv_amd import load_params
from fpyv_amd.clouds import PointCloud
from fpyv_amd.env import DroneBatch, FpvVecEnv, RacerBatch
from fpyv_amd.objects import Cylinder, Gate, Ground, Target
from fpyv_amd.splat import PointCloudCamera

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NMAX = 130
GUARD = 0x5A
PAD = 8                     # elements behind every image, rows behind centroid and lit


def _bits(a):
    a = np.ascontiguousarray(a.cpu().numpy() if torch.is_tensor(a) else a)
    return a.view(np.uint32) if a.dtype.itemsize == 4 else a.view(np.uint8)


@functools.lru_cache(maxsize=None)
def _scene():
    """(position, ypr) of NMAX drones within 15 m of the origin at every attitude; computed once, read-only"""
    rng = np.random.default_rng(23)
    pos = np.stack([rng.uniform(-15, 15, NMAX), rng.uniform(-15, 15, NMAX), rng.uniform(0.3, 8.0, NMAX)], 1)
    ypr = np.stack([rng.uniform(-40, 40, NMAX), rng.uniform(-40, 40, NMAX), rng.uniform(-180, 180, NMAX)], 1)
    ypr[2] = [180.0, 0.0, 30.0]                              # inverted
    return pos.astype(np.float32), ypr.astype(np.float32)


@functools.lru_cache(maxsize=None)
def _cloud(sizes=(0, 1, 255, 256, 257, 1000), pad=True):
    """objects of the given point counts - balls of points among the drones - with NaN in a padded point_ld; computed once"""
    rng = np.random.default_rng(sum(sizes) + len(sizes))
    clouds = []
    for s in sizes:
        c = np.array([rng.uniform(-12, 12), rng.uniform(-12, 12), rng.uniform(0, 6)])
        clouds.append(c + rng.normal(0, 1.5, (s, 3)))
    cl = PointCloud(clouds)
    if pad:
        cl.points = np.ascontiguousarray(np.concatenate([cl.points, np.full((3, PAD), np.nan, dtype=np.float32)], axis=1))
        cl.point_ld += PAD
    return cl


def _batch(n, cls=DroneBatch, **kw):
    b = cls(None if cls is RacerBatch else load_params(fps=250), n, device=DEV, **kw)
    if cls is DroneBatch:
        pos, ypr = _scene()
        b.reset(position=pos[:n], ypr=ypr[:n])
    else:
        b.reset()
    return b


def _pose(b):
    s = b.state[:10, :b.n].cpu().numpy()
    return s[0:3].T.copy(), s[6:10].T.copy()


def _raw(b, cam, cloud):
    """One render of batch b through a struct of the test's own: a padded image_ld, guard bytes behind every image, behind centroid and
    lit.  Checks the guards and returns (image [n, H, W], centroid, lit) as numpy."""
    n = b.n
    w, h = cam.resolution
    s = cam.derive()
    cloud.fill(s)
    pts = torch.from_numpy(cloud.points).to(DEV)
    s.points = pts.data_ptr()
    size = 4 if cam.encoding == "metres" else 1
    ld = w * h + PAD
    img = torch.full((n, ld * size), GUARD, dtype=torch.uint8, device=DEV)
    s.image, s.image_ld = img.data_ptr(), ld
    cen = lit = None
    if cam.centroid:
        cen = torch.full((n + PAD, 8), GUARD, dtype=torch.uint8, device=DEV)
        lit = torch.full((n + PAD, 4), GUARD, dtype=torch.uint8, device=DEV)
        s.centroid, s.lit = cen.data_ptr(), lit.data_ptr()
    b._sensor_raw(b._L.fpv_splat_render, s, None)
    torch.cuda.synchronize()
    assert torch.all(img[:, w * h * size:] == GUARD), "image padding"
    image = img[:, :w * h * size].cpu().numpy()
    image = image.view(np.float32).reshape(n, h, w) if size == 4 else image.reshape(n, h, w)
    if cen is not None:
        assert torch.all(cen[n:] == GUARD) and torch.all(lit[n:] == GUARD), "behind centroid / lit"
        cen, lit = cen[:n].cpu().numpy().view(np.float32).reshape(n, 2), lit[:n].cpu().numpy().view(np.int32).reshape(n)
    return image, cen, lit


def _same(got, want):
    image, cen, lit = got
    assert np.array_equal(_bits(image), _bits(want["image"])), "image"
    if want["centroid"] is not None:
        assert np.array_equal(_bits(cen), _bits(want["centroid"])), "centroid"
        assert np.array_equal(lit, want["lit"]), "lit"


# ---- 1. bit identity ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res", [(4, 4), (8, 8), (12, 8), (64, 48), (128, 128)])
def test_kernel_equals_evaluate_bit_for_bit_at_every_size(res):
    """every image size up to the LDS limit, 1 / 3 / 130 drones, the three encodings, objects of 0, 1, 255, 256, 257 and 1000 points"""
    cl = _cloud()
    lit_any = False
    for n in (1, 3, 130):
        b = _batch(n)
        p, q = _pose(b)
        for enc in ("u8", "metres", "mask"):
            cam = PointCloudCamera(resolution=res, encoding=enc, centroid=(enc != "mask"))
            want = cam.evaluate(p, q, cl, image_ld=res[0] * res[1] + PAD)
            _same(_raw(b, cam, cl), want)
            lit_any = lit_any or bool((want["image"] > 0).any() if enc != "metres" else (want["image"] < 25.0).any())
        b.close()
    assert lit_any


def test_one_object_and_72_and_worlds_nobody_sees():
    n = 33
    b = _batch(n)
    p, q = _pose(b)
    cam = PointCloudCamera(resolution=(16, 12), centroid=True)
    for cl in (_cloud((300,)), _cloud(tuple([0, 5, 40, 64, 65, 130] * 12)), PointCloud([])):
        want = cam.evaluate(p, q, cl, image_ld=16 * 12 + PAD)
        _same(_raw(b, cam, cl), want)
    assert _cloud(tuple([0, 5, 40, 64, 65, 130] * 12)).count == 72
    # every object pruned: the world 4 km below level drones (every corner of every box is behind the camera)
    rng = np.random.default_rng(3)
    far = PointCloud([rng.normal(0, 1.0, (200, 3)) + [0.0, 0.0, -4000.0 - 100 * k] for k in range(5)])
    up = _batch(n)
    up.state[6:10, :n] = torch.tensor([[1.0], [0.0], [0.0], [0.0]], device=DEV)            # level: the camera looks up and ahead
    up.state[6:10, 1] = torch.tensor([0.9238795, 0.0, 0.0, 0.3826834], device=DEV)          # ... lane 1 turned 45 degrees about z
    p, q = _pose(up)
    want = cam.evaluate(p, q, far, image_ld=16 * 12 + PAD)
    assert not want["image"].any() and np.isnan(want["centroid"]).all() and not want["lit"].any()
    _same(_raw(up, cam, far), want)
    # every point behind the camera (camera angle 0: it looks along the body's x): a wall behind lane 0, and two points behind lane 1
    # whose box has a corner in front of it - kept, and nothing lands
    cam0 = PointCloudCamera(resolution=(16, 12), camera_angle=0.0, position_relative_to_frame=(0, 0, 0), centroid=True, encoding="mask")
    wall = np.stack([np.full(400, -5.0), rng.uniform(-50, 50, 400), rng.uniform(-50, 50, 400)], 1) + p[0]
    pair = np.array([[10.0, -20.0, 0.0], [-20.0, 10.0, 0.0]]) + p[1]
    behind = PointCloud([wall, pair])
    want = cam0.evaluate(p[:2], q[:2], PointCloud([wall]), image_ld=16 * 12 + PAD)
    assert not want["image"][0].any()
    want = cam0.evaluate(p[:2], q[:2], PointCloud([pair]), image_ld=16 * 12 + PAD)
    assert not want["image"][1].any()
    _same(_raw(up, cam0, behind), cam0.evaluate(p, q, behind, image_ld=16 * 12 + PAD))
    _same(_raw(b, cam0, behind), cam0.evaluate(*_pose(b), behind, image_ld=16 * 12 + PAD))
    b.close(); up.close()


def test_many_points_in_one_pixel_and_the_column_0_quirk():
    """camera angle 0 at the body's origin, a level drone at the origin: camera-frame points are placed pixel by pixel"""
    w, h = 16, 12
    cam = PointCloudCamera(resolution=(w, h), camera_angle=0.0, position_relative_to_frame=(0, 0, 0), max_depth=25.0, encoding="metres")
    s = cam.derive()
    f, R = float(s.focal_length), np.array(s.relative_rotation[:]).reshape(3, 3)

    def at(u, v, z):                                         # the world point that projects to (u, v) at depth z
        return R @ np.array([(u - w / 2) / f * z, (v - h / 2) / f * z, z])

    rng = np.random.default_rng(8)
    same_depth = [at(5.5, 3.5, 7.0)] * 300                                                  # 300 points, one pixel, one depth
    depths = rng.uniform(2.0, 20.0, 700)
    pile = [at(9.2 + rng.uniform(0, 0.6), 6.2 + rng.uniform(0, 0.6), z) for z in depths]    # 700 depths, one pixel
    quirk = [at(-0.5, 4.5, 3.0), at(6.5, -0.5, 4.0), at(-1.5, 5.5, 3.0)]                    # (-1, 0) lands in column / row 0; -1.5 is out
    cl = PointCloud([np.array(same_depth), np.array(pile), np.array(quirk)])
    b = _batch(3)
    b.state[0:3, :3] = 0.0
    b.state[6:10, :3] = torch.tensor([[1.0], [0.0], [0.0], [0.0]], device=DEV)
    p, q = _pose(b)
    want = cam.evaluate(p, q, cl, image_ld=w * h + PAD)
    img = want["image"][0]
    assert abs(img[3, 5] - 7.0) < 1e-4 and abs(img[6, 9] - depths.min()) < 1e-4
    assert abs(img[4, 0] - 3.0) < 1e-4 and abs(img[0, 6] - 4.0) < 1e-4 and img[5, 0] == 25.0
    assert (img < 25.0).sum() == 4
    _same(_raw(b, cam, cl), want)
    b.close()


# ---- 2. the batch: a moved Target, moved gates, the stepper left alone ----------------------------------------------------------
def test_a_moved_target_changes_the_offset_only_and_set_gates_rebuilds_the_gates():
    n = 40
    target = Target([6.0, 0.0, 4.0], 1.0, 3, path=dict(radius=3.0, resolution=12))
    ground = Ground(40, 30)
    th = np.deg2rad(30.0)
    gates = [Gate([8.0, 2.0, 3.0], np.array([[np.cos(th), -np.sin(th), 0.0], [np.sin(th), np.cos(th), 0.0], [0.0, 0.0, 1.0]]), 2.5, shape="circle")]
    cam = PointCloudCamera(resolution=(32, 24), centroid=True)
    b = _batch(n, gates=gates, cloud_camera=cam)
    before, steps = b.state.clone(), b.step_counter()
    out = b.render_points([ground, target])
    torch.cuda.synchronize()
    assert out.data_ptr() == b.points_image.data_ptr() and out.shape == (n, 24, 32) and out.dtype == torch.uint8
    assert torch.equal(b.state, before) and b.step_counter() == steps                       # the stepper is left alone
    p, q = _pose(b)
    want = cam.evaluate(p, q, PointCloud.from_world([ground, target], gates))
    _same((out.cpu().numpy(), b.points_centroid.cpu().numpy(), b.points_lit.cpu().numpy()), want)
    assert want["lit"].any() and b._cloud.count == 3
    uploaded, cloud = b._cloud_dev, b._cloud
    target.update(); target.update()
    b.render_points([ground, target])                                                       # the same objects: no new cloud, no upload
    torch.cuda.synchronize()
    assert b._cloud_dev is uploaded and b._cloud is cloud
    moved = cam.evaluate(p, q, PointCloud.from_world([ground, target], gates))
    assert not np.array_equal(moved["image"], want["image"])
    _same((b.points_image.cpu().numpy(), b.points_centroid.cpu().numpy(), b.points_lit.cpu().numpy()), moved)
    b.render_points()                                                                       # None: the last world again
    torch.cuda.synchronize()
    assert np.array_equal(b.points_image.cpu().numpy(), moved["image"])
    raised = [Gate(np.asarray(g.position) + [0.0, 0.0, 1.5], g.rotation_matrix, g.size, shape=g.shape) for g in gates]
    b.set_gates(raised)
    b.render_points([ground, target])
    torch.cuda.synchronize()
    again = cam.evaluate(p, q, PointCloud.from_world([ground, target], raised))
    assert b._cloud is not cloud and not np.array_equal(again["image"], moved["image"])
    _same((b.points_image.cpu().numpy(), b.points_centroid.cpu().numpy(), b.points_lit.cpu().numpy()), again)
    # a ready PointCloud is taken as it is; the Racer renders the same poses alike
    r = _batch(n, cls=RacerBatch, cloud_camera=cam)
    r.state[0:3, :n] = b.state[0:3, :n]; r.state[6:10, :n] = b.state[6:10, :n]
    r.render_points(PointCloud.from_world([ground, target], raised))
    torch.cuda.synchronize()
    assert np.array_equal(r.points_image.cpu().numpy(), again["image"])
    with pytest.raises(ValueError, match="without cloud_camera="):
        _batch(4).render_points([ground])
    b.close(); r.close()


# ---- 3. the reference on the device ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [0, 1])
def test_the_g23_poses_on_the_device_meet_the_capture_and_the_host(c):
    cap = L.load()
    n = cap["p"].shape[0]
    cam = L.camera(cap, c, centroid=True)
    b = DroneBatch(load_params(fps=250), n, device=DEV, cloud_camera=cam)
    b.reset()
    b.state[0:3, :n] = torch.from_numpy(cap["p"].T.astype(np.float32)).to(DEV)
    b.state[6:10, :n] = torch.from_numpy(cap["q"].T.astype(np.float32)).to(DEV)
    b.render_points(L.scene(cap))
    torch.cuda.synchronize()
    got = b.points_image.cpu().numpy()
    hard, soft = L.fragile(cap, c)
    assert L.compare(cap, c, got, cap[f"image{c}"], hard, soft) >= 0.98 * hard.size
    host = cam.evaluate(cap["p"], cap["q"], L.cloud(cap))
    _same((got, b.points_centroid.cpu().numpy(), b.points_lit.cpu().numpy()), host)
    b.close()


# ---- 4. the env -----------------------------------------------------------------------------------------------------------------
def _env(parts, every):
    rng = np.random.default_rng(11)
    objs = [Ground(40, 24), Cylinder([4.0, 3.0, 0.0], 1.0, 5.0, 17, 9), Target([-5.0, 2.0, 3.0], 0.8, 2)]
    gates = [Gate([9.0, -3.0, 3.0], np.eye(3), 2.0, shape="rectangle"), Gate([-8.0, 6.0, 2.5], np.eye(3), 2.0, shape="half_circle")]
    env = FpvVecEnv(load_params(fps=250, ceiling=6.0), num_envs=300, device=DEV, auto_reset=True, object_list=objs, gates=gates, partitions=parts,
                    cloud_camera=PointCloudCamera(resolution=(16, 12), centroid=True), cloud_every=every)
    pos = np.stack([rng.uniform(-8, 8, 300), rng.uniform(-8, 8, 300), rng.uniform(4.0, 5.9, 300)], 1).astype(np.float32)
    vel = np.stack([rng.uniform(-1, 1, 300), rng.uniform(-1, 1, 300), rng.uniform(2.0, 9.0, 300)], 1).astype(np.float32)
    env.reset(position=pos, velocity=vel)
    return env


def test_env_with_partitions_equals_the_unpartitioned_env_and_cloud_every_zero_waits():
    one, two, never = _env(1, 2), _env(2, 2), _env(1, 0)
    torch.cuda.synchronize()
    assert two.partitions == 2 and one.points_image.shape == (300, 12, 16) and one.points_image.any()       # rendered after the reset
    assert not never.points_image.any()                                                                     # cloud_every=0: not even then
    sticks = torch.from_numpy(np.random.default_rng(5).uniform(-0.2, 0.2, (12, 300, 4)).astype(np.float32)).to(DEV)
    sticks[..., 3] = 0.8
    resets = 0
    cam = one.batch.cloud_camera

    def host(env):
        s = env.batch.state[:10, :300].cpu().numpy()
        return cam.evaluate(s[0:3].T, s[6:10].T, PointCloud.from_world(env.object_list, env.batch._gate_list))

    for t in range(12):
        _, _, done, info = one.step(sticks[t])
        _, _, done2, info2 = two.step(sticks[t])
        never.step(sticks[t])
        torch.cuda.synchronize()
        resets += int(done.sum())
        assert torch.equal(done, done2)
        for a, b in ((one.points_image, two.points_image), (one.points_centroid, two.points_centroid), (one.points_lit, two.points_lit)):
            assert np.array_equal(_bits(a), _bits(b)), t
        assert info["points_image"].data_ptr() == one.points_image.data_ptr() and info2["points_centroid"].shape == (300, 2)
        if t % 2 == 1:                                     # rendered after this step: the image belongs to obs, auto-reset lanes included
            want = host(one)
            _same((one.points_image.cpu().numpy(), one.points_centroid.cpu().numpy(), one.points_lit.cpu().numpy()), want)
    assert resets > 10 and not never.points_image.any()
    got = never.render_points()
    torch.cuda.synchronize()
    assert np.array_equal(got.cpu().numpy(), host(never)["image"])
    every = _env(2, 1)
    every.step(sticks[0])
    torch.cuda.synchronize()
    assert np.array_equal(every.points_image.cpu().numpy(), host(every)["image"])
    for e in (one, two, never, every):
        e.close()


# ---- 5. inputs no flight visits -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("enc", ["u8", "metres"])
def test_poses_no_flight_visits_match_the_host_and_stay_inside_their_image(enc):
    n = 12
    cam = PointCloudCamera(resolution=(16, 12), camera_angle=0.0, position_relative_to_frame=(0, 0, 0), encoding=enc, centroid=True)
    b = _batch(n)
    st = b.state
    st[0:3, :n] = torch.tensor([[0.0], [0.0], [5.0]], device=DEV)
    st[6:10, :n] = torch.tensor([[1.0], [0.0], [0.0], [0.0]], device=DEV)          # the camera looks along +x from (0, 0, 5)
    nan, inf = float("nan"), float("inf")
    st[0, 1], st[1, 2], st[2, 3] = nan, inf, -inf                                  # NaN and Inf in the position
    st[6:10, 4] = torch.tensor([2.0, 0.0, 0.0, 0.0], device=DEV)                   # a non-unit quaternion
    st[6:10, 5] = 0.0                                                              # the zero quaternion
    st[6:10, 6] = torch.tensor([nan, 0.0, 0.0, 0.0], device=DEV)
    st[0, 7], st[6:10, 8] = 1.0e30, torch.tensor([0.3, -0.7, 2.5, 1.0e19], device=DEV)
    st[0:3, 9] = torch.tensor([1.0e38, -1.0e38, 1.0e38], device=DEV)               # differences that overflow
    st[6:10, 10] = torch.tensor([inf, 0.0, 0.0, 0.0], device=DEV)
    rng = np.random.default_rng(17)
    near = np.stack([rng.uniform(2, 12, 500), rng.uniform(-6, 6, 500), rng.uniform(0, 10, 500)], 1)
    huge = np.array([[1.0e30, 0.0, 5.0], [3.0e38, 3.0e38, 3.0e38], [5.0, 1.0e-30, 5.0], [0.0, 0.0, 5.0], [1.0e-38, 0.0, 5.0]])
    cl = PointCloud([near, huge, near[:64] * [1.0, -1.0, 1.0]])
    p, q = _pose(b)
    want = cam.evaluate(p, q, cl, image_ld=16 * 12 + PAD)
    _same(_raw(b, cam, cl), want)                                                  # (_raw checks the guards behind every image)
    assert want["lit"][0] > 0 and want["lit"][1] == 0 and np.isnan(want["centroid"][1]).all() and want["lit"][6] == 0
    b.close()
