"""The env with everything attached that tests/test_gpu_attachments.py and tests/test_gpu_resume.py share: the lists of a batch's and an
env's public tensors that the sensors and the task write, the bitwise comparison, the world and the env's factory.  Nothing here is
used by the product."""
import numpy as np

from fpyv_amd import load_params
from fpyv_amd.camera import DepthCamera
from fpyv_amd.detect import BoxDetector
from fpyv_amd.env import FpvVecEnv
from fpyv_amd.objects import Cylinder, Gate, Ground, Target
from fpyv_amd.pursuit import PursuitTask
from fpyv_amd.splat import PointCloudCamera

DEV = "cuda:0"
N = 384
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
GATES = ([9.0, -3.0, 3.0], "rectangle"), ([-8.0, 6.0, 2.5], "half_circle")


def bits(t):
    a = np.ascontiguousarray(t.cpu().numpy() if hasattr(t, "cpu") else t)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def world():
    target = Target([-5.0, 2.0, 3.0], 0.8, 2, path=dict(radius=3.0, resolution=12))
    return [Ground(40, 24), Cylinder([4.0, 3.0, 0.0], 1.0, 5.0, 17, 9), target], target


def task_and_starts(n=N):
    """(the pursuit task, start positions, start velocities) of the env below: one seeded stream"""
    rng = np.random.default_rng(31)
    targets = dict(centre=np.stack([rng.uniform(-6, 6, n), rng.uniform(-6, 6, n), rng.uniform(1, 5, n)], 1).astype(np.float32),
                   radius=rng.uniform(0.3, 0.8, n).astype(np.float32), path_radius=rng.uniform(0.5, 4.0, n).astype(np.float32),
                   phase=rng.integers(0, 29, n))
    task = PursuitTask(targets=targets, path=dict(radius=2.0, resolution=29), capture_distance=0.25, obs=True, guide=dict(max_depth=40.0),
                       respawn=dict(lo=(-6.0, -6.0, 1.0), hi=(6.0, 6.0, 5.0), radius=(0.3, 0.8), seed=77))
    pos = np.stack([rng.uniform(-8, 8, n), rng.uniform(-8, 8, n), rng.uniform(4.0, 5.9, n)], 1).astype(np.float32)
    vel = np.stack([rng.uniform(-1, 1, n), rng.uniform(-1, 1, n), rng.uniform(2.0, 9.0, n)], 1).astype(np.float32)
    return task, pos, vel


def env(objs, parts, n=N, every=(2, 3, 2), gates=True, **kw):
    """(env, start positions, start velocities) of `n` drones with everything attached; `every` = (depth, detect, cloud)_every.
    gates=False leaves the course out (what guided=True needs: the library refuses a course under the guidance override); `kw`
    goes to the env."""
    task, pos, vel = task_and_starts(n)
    course = [Gate(c, np.eye(3), 2.0, shape=shape) for c, shape in GATES] if gates else None
    e = FpvVecEnv(load_params(fps=250, ceiling=6.0), num_envs=n, device=DEV, auto_reset=True, object_list=objs, gates=course, partitions=parts,
                  range_rays=[[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, -1.0]], depth_camera=DepthCamera(resolution=(8, 4)),
                  detector=BoxDetector(own_target=True), cloud_camera=PointCloudCamera(resolution=(8, 4), centroid=True), pursuit=task,
                  depth_every=every[0], detect_every=every[1], cloud_every=every[2], **kw)
    return e, pos, vel
