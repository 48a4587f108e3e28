"""Every sensor and the pursuit task on one env at once: range rays, depth camera, box detector with the own-target slot, point-cloud
camera with its centroid, a guided pursuit task and a gate course, each on its own cadence, with in-kernel auto-resets, a masked
reset and a moving Target.  384 drones in two partitions are the column ranges [0, 128) and [128, 384): a pointer of a partition
moved by the wrong step lands in the other one's columns.  The unpartitioned env, the env with partitions=2 driven by step() and a
third one driven by step_async / step_wait agree BIT FOR BIT after every call - obs, reward, done, every sensor output and every
info entry -, and what step_wait(k) hands out is the [lo:hi] slice of the whole population's entry."""
import numpy as np
import pytest
import torch

from fpyv_amd import load_params
from fpyv_amd.camera import DepthCamera
from fpyv_amd.detect import BoxDetector
from fpyv_amd.env import FpvVecEnv
from fpyv_amd.objects import Cylinder, Gate, Ground, Target
from fpyv_amd.pursuit import PursuitTask
from fpyv_amd.splat import PointCloudCamera

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, STEPS, RESET_AFTER = 384, 7, 3
# the public tensors of the batch that the sensors and the task write
OUTPUTS = ("range_rows", "depth", "box_rows", "box_depth_rows", "box_visible_rows", "points_image", "points_centroid", "points_lit",
           "target_rows", "target_obs_rows", "target_position_rows", "target_event_u8", "pursuit_reward", "pursuit_pid_rows",
           "gate_word", "gate_obs_rows", "ep_return", "last_return", "last_length")
# the views of the env
VIEWS = ("ranges", "depth", "boxes", "box_depth", "box_visible", "points_image", "points_centroid", "points_lit", "target_obs",
         "target_position", "target_event", "captures", "gate_obs")
INFO_KEYS = {"episode_return", "episode_length", "gates_passed", "gate_event", "target_obs", "target_event", "captures", "ranges", "depth",
             "boxes", "box_depth", "box_visible", "points_image", "points_centroid"}
COLUMNS_LAST = ("ranges", "boxes", "box_depth", "box_visible")           # info entries whose drones are the last axis; the others' the first


def _bits(t):
    a = np.ascontiguousarray(t.cpu().numpy())
    return a.view({1: np.uint8, 4: np.uint32}[a.dtype.itemsize])


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


def _world():
    target = Target([-5.0, 2.0, 3.0], 0.8, 2, path=dict(radius=3.0, resolution=12))
    return [Ground(40, 24), Cylinder([4.0, 3.0, 0.0], 1.0, 5.0, 17, 9), target], target


def _env(objs, parts, n=N, every=(2, 3, 2)):
    """(env, start positions, start velocities) of `n` drones with everything attached; `every` = (depth, detect, cloud)_every"""
    rng = np.random.default_rng(31)
    gates = [Gate([9.0, -3.0, 3.0], np.eye(3), 2.0, shape="rectangle"), Gate([-8.0, 6.0, 2.5], np.eye(3), 2.0, shape="half_circle")]
    targets = dict(centre=np.stack([rng.uniform(-6, 6, n), rng.uniform(-6, 6, n), rng.uniform(1, 5, n)], 1).astype(np.float32),
                   radius=rng.uniform(0.3, 0.8, n).astype(np.float32), path_radius=rng.uniform(0.5, 4.0, n).astype(np.float32),
                   phase=rng.integers(0, 29, n))
    task = PursuitTask(targets=targets, path=dict(radius=2.0, resolution=29), capture_distance=0.25, obs=True, guide=dict(max_depth=40.0),
                       respawn=dict(lo=(-6.0, -6.0, 1.0), hi=(6.0, 6.0, 5.0), radius=(0.3, 0.8), seed=77))
    env = FpvVecEnv(load_params(fps=250, ceiling=6.0), num_envs=n, device=DEV, auto_reset=True, object_list=objs, gates=gates, partitions=parts,
                    range_rays=[[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, -1.0]], depth_camera=DepthCamera(resolution=(8, 4)),
                    detector=BoxDetector(own_target=True), cloud_camera=PointCloudCamera(resolution=(8, 4), centroid=True), pursuit=task,
                    depth_every=every[0], detect_every=every[1], cloud_every=every[2])
    pos = np.stack([rng.uniform(-8, 8, n), rng.uniform(-8, 8, n), rng.uniform(4.0, 5.9, n)], 1).astype(np.float32)
    vel = np.stack([rng.uniform(-1, 1, n), rng.uniform(-1, 1, n), rng.uniform(2.0, 9.0, n)], 1).astype(np.float32)
    return env, pos, vel


def _whole(env, one, what):
    """every output of `env` is the unpartitioned env's, bit for bit"""
    torch.cuda.synchronize()
    assert _same(env.obs, one.obs) and _same(env.batch.reward, one.batch.reward) and _same(env.batch.done, one.batch.done), what
    for name in OUTPUTS:
        assert _same(getattr(env.batch, name), getattr(one.batch, name)), (what, name)
    for g, h in zip(env.batch.pursuit_guidance, one.batch.pursuit_guidance):
        assert _same(g, h), what
    for name in VIEWS:
        assert _same(getattr(env, name), getattr(one, name)), (what, name)


def _results(got, want, what, lo=None, hi=None):
    """a step's (obs, reward, done, info) is another's - or, with [lo, hi), that range of its columns - bit for bit, key for key"""
    cut = (lambda t, last=False: t) if lo is None else (lambda t, last=False: t[..., lo:hi] if last else t[lo:hi])
    for a, b in zip(got[:3], want[:3]):
        assert _same(a, cut(b)), what
    assert set(got[3]) == set(want[3]) == INFO_KEYS, what
    for key in INFO_KEYS:
        assert _same(got[3][key], cut(want[3][key], key in COLUMNS_LAST)), (what, key)


def test_partitions_and_split_phase_change_no_bit_of_an_env_with_every_attachment():
    objs, target = _world()
    (one, pos, vel), (two, _, _), (split, _, _) = _env(objs, 1), _env(objs, 2), _env(objs, 2)
    assert two.partitions == 2 and [split.partition_range(k) for k in (0, 1)] == [(0, 128), (128, 384)]
    for e in (one, two, split):
        e.reset(position=pos, velocity=vel)
    _whole(two, one, "reset"); _whole(split, one, "reset")
    sticks = torch.from_numpy(np.random.default_rng(5).uniform(-0.2, 0.2, (STEPS, N, 4)).astype(np.float32)).to(DEV)
    sticks[..., 3] = 0.8
    mask = torch.arange(N, device=DEV) % 3 == 0
    resets = 0
    for t in range(STEPS):
        target.update()
        want = one.step(sticks[t])
        _results(two.step(sticks[t]), want, t)
        for k in (0, 1):
            lo, hi = split.partition_range(k)
            split.step_async(k, sticks[t, lo:hi])
        parts = {k: split.step_wait(k) for k in (1, 0)}
        torch.cuda.synchronize()
        for k, got in parts.items():
            _results(got, want, (t, k), *split.partition_range(k))
        _whole(two, one, t); _whole(split, one, t)
        resets += int(want[2].sum())
        if t + 1 == RESET_AFTER:
            for e in (one, two, split):
                e.reset(mask)
            _whole(two, one, "masked reset"); _whole(split, one, "masked reset")
    assert resets > 10 and one.batch.range_rows.any() and one.depth.any() and one.box_visible.any() and one.points_image.any()
    target.update()
    for call in ("render_depth", "detect", "render_points"):
        outs = [getattr(e, call)() for e in (one, two, split)]
        _whole(two, one, call); _whole(split, one, call)
        assert _same(outs[1], outs[0]) and _same(outs[2], outs[0]), call
    for e in (one, two, split):
        e.close()
