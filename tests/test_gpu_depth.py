"""The depth camera on the GPU (include/fpv_abi.h "Depth camera"): every comparison is bit for bit against
DepthCamera.evaluate - the kernel's own pixel function on the host - on the positions and attitudes read back from the batch."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import depth_scene as S
import gate_course as gc
from conftest import REPO
from fpyv_amd import _lib, load_params, sticks
from fpyv_amd.camera import DepthCamera
from fpyv_amd.env import DroneBatch, FpvVecEnv, RacerBatch
from fpyv_amd.objects import Gate, Target

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NMAX = 130


def _bits(a):
    a = np.ascontiguousarray(a)
    return a if a.dtype == np.uint8 else a.view(np.uint32)


def _pose(batch):
    s = batch.state[:10, :batch.n].cpu().numpy()
    return s[0:3].T.copy(), s[6:10].T.copy()


def _expect(batch, objects, gates=()):
    p, q = _pose(batch)
    return batch.depth_camera.evaluate(p, q, objects, gates)


def _scattered(n, seed=2):
    rng = np.random.default_rng(seed)
    pos = np.stack([rng.uniform(-8, 8, n), rng.uniform(-8, 8, n), rng.uniform(0.5, 7, n)], 1)
    return pos, rng.uniform(-3, 3, (n, 3)), rng.uniform(-180, 180, (n, 3)) * np.array([0.2, 0.2, 1.0])


@functools.lru_cache(maxsize=None)
def _flown_state():
    """[14, NMAX] fp32: scattered per-drone starts flown for 50 steps with EMA sticks.  Computed once; treat as read-only."""
    b = DroneBatch(load_params(fps=1000), NMAX, device=DEV)
    pos, vel, ypr = _scattered(NMAX)
    b.reset(position=pos, velocity=vel, ypr=ypr)
    a = torch.from_numpy(sticks.ema_noise(50, range(NMAX), seed=3)).to(DEV)
    for t in range(50):
        b.step(a[t], return_imu=False)
    torch.cuda.synchronize()
    return b.state[:, :NMAX].cpu().numpy()


@functools.lru_cache(maxsize=None)
def _poses_that_see_gates(res):
    """The flown states with the drones whose `res` image shows most of the 64-gate course first, so that the gates are in the
    picture of every population down to one drone: [14, NMAX] fp32 and the number of drones that see a gate frame at all."""
    st = _flown_state()
    cam = DepthCamera(resolution=res, max_depth=S.MAX_DEPTH)
    p, q = st[0:3].T.copy(), st[6:10].T.copy()
    frames = (cam.evaluate(p, q, S.world(4), S.course(64)) != cam.evaluate(p, q, S.world(4))).reshape(NMAX, -1).sum(1)
    order = np.argsort(-frames, kind="stable")
    return np.ascontiguousarray(st[:, order]), int((frames > 0).sum())


# ---- T1: image sizes, populations, encodings and worlds ---------------------------------------------------------------------------
# 4 x 4: a quarter-filled wave; 8 x 8: one wave; 12 x 8: a ragged second wave; 64 x 48: 48 waves.  n = 1, 3, 5, 130: blocks (four
# waves) span drones and end ragged.
@pytest.mark.parametrize("res", [(4, 4), (8, 8), (12, 8), (64, 48)])
@pytest.mark.parametrize("n", [1, 3, 5, 130])
def test_render_equals_the_host_function_for_every_size_encoding_and_world(n, res):
    course = S.course(64)
    state, seeing = _poses_that_see_gates(res)
    assert seeing >= 5                                       # every population below starts with drones that see a gate frame
    for enc in ("metres", "u8"):
        cam = DepthCamera(resolution=res, max_depth=S.MAX_DEPTH, encoding=enc)
        plain = DroneBatch(load_params(fps=1000), n, device=DEV, depth_camera=cam)
        gated = DroneBatch(load_params(fps=1000), n, device=DEV, depth_camera=cam, gates=course)
        for b in (plain, gated):
            b.state[:, :n].copy_(torch.from_numpy(state[:, :n]).to(DEV))
            assert b.depth.shape == (n, res[1], res[0]) and b.depth.dtype == (torch.uint8 if enc == "u8" else torch.float32)
        for count in (0, 4, 8):
            plain.depth.fill_(7)
            got = plain.render_depth(S.world(count))
            assert got.data_ptr() == plain.depth.data_ptr()
            assert np.array_equal(_bits(got.cpu().numpy()), _bits(_expect(plain, S.world(count)))), (n, res, enc, count)
        gated.depth.fill_(7)
        got = gated.render_depth(S.world(4)).cpu().numpy()
        want = _expect(gated, S.world(4), course)
        assert np.array_equal(_bits(got), _bits(want)), (n, res, enc, "64 gates")
        if enc == "metres":                                  # the gates are in the picture: the kernel's gate loop counts
            assert (want != _expect(gated, S.world(4))).reshape(n, -1).any(1)[:min(n, seeing)].all(), (n, res)
        # a stride larger than W * H leaves its padding unwritten
        px = res[0] * res[1]
        wide = torch.full((n, px + 8), 7, dtype=gated.depth.dtype, device=DEV)
        r = _lib.FpvDepthRender.from_buffer_copy(gated._render)
        r.image, r.image_stride = wide.data_ptr(), px + 8
        gated._depth_render_raw(r)
        wide = wide.cpu().numpy()
        assert np.array_equal(_bits(wide[:, :px].reshape(want.shape)), _bits(want)) and (wide[:, px:] == 7).all()


# ---- T2: the render leaves the handle alone -----------------------------------------------------------------------------------------
def _pair(kind, cam):
    p = load_params(fps=1000)
    kw, cls = dict(auto_reset=True), DroneBatch
    if kind == "physics":
        kw.update(per_drone_physics=True)
    elif kind == "gates":
        kw.update(gates=gc.course(), laps=1)
    elif kind == "noise":
        kw.update(stick_noise=True, noise_seed=5)
    elif kind == "reset_pose":
        kw.update(per_drone_reset_pose=True)
    elif kind == "racer":
        cls = RacerBatch
    a, b = cls(p, 260, device=DEV, **kw), cls(p, 260, device=DEV, depth_camera=cam, **kw)
    for x in (a, b):
        if kind == "racer":
            x.reset()
        else:
            pos, vel, ypr = _scattered(260, seed=4)
            x.reset(position=pos, velocity=vel, ypr=ypr)
        if kind == "physics":
            x.randomize_physics(7, mass=(0.8, 1.2))
    return a, b


@pytest.mark.parametrize("kind", ["plain", "physics", "gates", "noise", "reset_pose", "racer"])
def test_a_chain_with_renders_ends_where_the_chain_without_them_ends(kind):
    cam = DepthCamera(resolution=(16, 12), max_depth=S.MAX_DEPTH)
    plain, seeing = _pair(kind, cam)
    world = S.world(4)
    n = plain.n
    if kind == "racer":
        rng = np.random.default_rng(6)
        acts = np.concatenate([rng.uniform(-2, 2, (20, n, 3)), rng.uniform(5, 12, (20, n, 1))], -1).astype(np.float32)
    else:
        acts = sticks.ema_noise(20, range(n), seed=8)
    a = torch.from_numpy(acts).to(DEV)
    for t in range(20):
        for x in (plain, seeing):
            x.step(a[t], return_imu=False)
        got = seeing.render_depth(world).cpu().numpy()
        if t % 5 == 4:
            assert np.array_equal(_bits(got), _bits(_expect(seeing, world, gc.course() if kind == "gates" else ()))), (kind, t)
    torch.cuda.synchronize()
    for name in ("state", "reward", "done", "noise_state", "gate_word"):
        x, y = getattr(plain, name, None), getattr(seeing, name, None)
        assert (x is None) == (y is None)
        if x is not None:
            assert torch.equal(x, y), (kind, name)
    assert plain.step_counter() == seeing.step_counter() == 20
    assert plain.rotation == seeing.rotation


# ---- T3: FpvVecEnv --------------------------------------------------------------------------------------------------------------
def _env(partitions=1, n=700, **kw):
    p = load_params(fps=1000).replace(init_position=np.array([0.0, 0.0, 1.0]), ceiling=1.02)
    cam = DepthCamera(resolution=(12, 8), max_depth=S.MAX_DEPTH, encoding=kw.pop("encoding", "metres"))
    return FpvVecEnv(p, num_envs=n, device=DEV, object_list=S.world(4), partitions=partitions, depth_camera=cam,
                     per_drone_reset_pose=True, gates=S.course(12), **kw)


def _env_expect(env):
    obs = env.obs.cpu().numpy()
    return env.batch.depth_camera.evaluate(obs[:, 0:3], obs[:, 6:10], env.object_list, S.course(12))


def test_env_depth_follows_obs_through_resets_and_auto_resets():
    env = _env()
    n = env.num_envs
    pos, vel, ypr = _scattered(n, seed=9)
    pos[:, 2] = 1.0 + 0.019 * np.arange(n) / n              # just under the ceiling: lanes reset at different steps
    env.reset(position=pos, velocity=vel * 0.1, ypr=ypr)
    assert np.array_equal(_bits(env.depth.cpu().numpy()), _bits(_env_expect(env)))
    a = torch.zeros((n, 4), device=DEV)
    a[:, 3] = 1.0                                          # full throttle: every lane reaches the ceiling and resets
    resets = 0
    for t in range(30):
        obs, reward, done, info = env.step(a)
        resets += int(done.sum())
        assert info["depth"].data_ptr() == env.depth.data_ptr() and env.depth.shape == (n, 8, 12)
        assert np.array_equal(_bits(env.depth.cpu().numpy()), _bits(_env_expect(env))), t
        back = done.cpu().numpy()
        if back.any():                                      # a lane that reset is back at ITS start: its image is the reset pose's
            assert np.allclose(obs.cpu().numpy()[back, 0:3], pos[back].astype(np.float32))
    assert resets > 0
    env.close()


def test_depth_every_renders_every_kth_step_and_never_with_zero():
    third, never = _env(depth_every=3, n=200), _env(depth_every=0, n=200)
    n = third.num_envs
    pos, vel, ypr = _scattered(n, seed=14)
    pos[:, 2] = 0.5
    for e in (third, never):
        e.depth.fill_(-1.0)
        e.reset(position=pos, velocity=vel, ypr=ypr)
    assert np.array_equal(_bits(third.depth.cpu().numpy()), _bits(_env_expect(third))) and (never.depth == -1.0).all()
    a = torch.from_numpy(sticks.ema_noise(6, range(n), seed=15)).to(DEV)
    for t in range(6):
        before = third.depth.clone()
        third.step(a[t]); never.step(a[t])
        if t % 3 == 2:
            assert np.array_equal(_bits(third.depth.cpu().numpy()), _bits(_env_expect(third))), t
        else:
            assert torch.equal(third.depth, before), t
    assert (never.depth == -1.0).all()
    got = never.render_depth()
    assert got.data_ptr() == never.depth.data_ptr() and np.array_equal(_bits(got.cpu().numpy()), _bits(_env_expect(never)))
    third.close(); never.close()


@pytest.mark.parametrize("encoding", ["metres", "u8"])
def test_partitions_give_the_same_bits(encoding):
    one, two = _env(1, encoding=encoding), _env(2, encoding=encoding)
    assert two.partitions == 2
    n = one.num_envs
    pos, vel, ypr = _scattered(n, seed=10)
    for e in (one, two):
        e.reset(position=pos, velocity=vel, ypr=ypr)
    a = torch.from_numpy(sticks.ema_noise(10, range(n), seed=12)).to(DEV)
    for t in range(10):
        one.step(a[t])
        for k in range(two.partitions):
            lo, hi = two.partition_range(k)
            two.step_async(k, a[t, lo:hi])
        for k in range(two.partitions):
            lo, hi = two.partition_range(k)
            obs, reward, done, info = two.step_wait(k)
            assert info["depth"].shape == (hi - lo, 8, 12)
        torch.cuda.synchronize()
        assert torch.equal(one.batch.state, two.batch.state) and torch.equal(one.depth, two.depth), t
    assert np.array_equal(_bits(two.depth.cpu().numpy()), _bits(_env_expect(two)))
    one.close(); two.close()


# ---- T4: moving things ------------------------------------------------------------------------------------------------------------
def test_a_moved_gate_and_a_moving_target_change_the_image_as_the_host_function_says():
    n = 150
    cam = DepthCamera(resolution=(16, 12), max_depth=S.MAX_DEPTH, gate_frame=0.4)
    b = DroneBatch(load_params(fps=1000), n, device=DEV, depth_camera=cam, gates=S.course(3))
    pos, vel, ypr = _scattered(n, seed=13)
    b.reset(position=pos, velocity=vel, ypr=ypr)
    target = Target([0.0, 0.0, 4.0], 1.5, path=dict(radius=4.0, resolution=12))
    a = torch.zeros((n, 4), device=DEV)
    seen = []
    for t in range(8):
        target.update()
        gates = [Gate(g.position + np.array([0.0, 0.0, 0.2 * t]), g.rotation_matrix, g.size, shape=g.shape) for g in S.course(3 + (t >= 4))[:3 + (t >= 4)]]
        b.set_gates(gates)                                   # moved up every step; a fourth gate joins half way
        b.step(a, object_list=[target], return_imu=False)
        got = b.render_depth().cpu().numpy()                 # None: the list the step bound
        assert np.array_equal(_bits(got), _bits(_expect(b, [target], gates))), t
        only_target = _expect(b, [target])
        assert (got != only_target).any(), t                 # the gates are in the picture
        seen.append(got)
    assert any(not np.array_equal(seen[0], s) for s in seen[1:]) and (seen[-1] < S.MAX_DEPTH).any()
    b.set_gates(None)                                        # no course bound: the gates are gone from the image
    assert np.array_equal(_bits(b.render_depth().cpu().numpy()), _bits(_expect(b, [target])))


# ---- T5: refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals_are_by_name_and_leave_the_next_step_working():
    p = load_params(fps=1000)
    n = 130
    cam = DepthCamera(resolution=(8, 8), max_depth=S.MAX_DEPTH)
    with pytest.raises(ValueError, match="built without depth_camera="):
        DroneBatch(p, n, device=DEV).render_depth()
    half = DroneBatch(p, n, device=DEV, fp16_state=True, depth_camera=cam)
    half.reset()
    with pytest.raises(_lib.FpvError, match="fp16 state"):
        half.render_depth()
    b = DroneBatch(p, n, device=DEV, depth_camera=cam)
    b.reset()
    for field, value, what in (("image_stride", 60, "image_stride is smaller"), ("image_stride", 66, "multiple of 4"), ("width", 2, "4..128"),
                               ("height", 200, "4..128"), ("width", 6, "multiple of 4"), ("max_depth", -1.0, "max_depth"),
                               ("max_depth", float("nan"), "max_depth"), ("image", None, "image is null"), ("struct_size", 16, "struct_size"),
                               ("encoding", 5, "encoding"), ("gate_count", 65, "gate_count"), ("gate_count", 2, "gates without descriptors")):
        s = _lib.FpvDepthRender.from_buffer_copy(b._render)
        setattr(s, field, value)
        with pytest.raises(_lib.FpvError, match=what):
            b._depth_render_raw(s)
    with pytest.raises(ValueError, match="at most 8"):
        b.render_depth([Target([k, 0, 0], 0.1) for k in range(9)])
    with pytest.raises(_lib.FpvError, match="4..128"):
        DroneBatch(p, n, device=DEV, depth_camera=DepthCamera(resolution=(256, 8)))
    a = torch.zeros((n, 4), device=DEV)
    for x in (b, half):
        x.step(a, return_imu=False)
    got = b.render_depth(S.world(4)).cpu().numpy()
    assert np.array_equal(_bits(got), _bits(_expect(b, S.world(4)))) and b.step_counter() == 1
    assert "depth" not in b.state_dict()                    # an output: checkpoints do not carry it


# ---- T6: the example ------------------------------------------------------------------------------------------------------------
def test_the_depth_camera_example_runs(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(REPO, "examples", "depth_camera.py"), "--drones", "256", "--steps", "20", "--out", str(tmp_path)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "pixels per second" in r.stdout
    img = np.load(os.path.join(str(tmp_path), "depth_0.npy"))
    assert img.shape == (48, 64) and (img < 25.0).any()
