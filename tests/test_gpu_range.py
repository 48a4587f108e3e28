"""The range sensor on the GPU (include/fpv_abi.h "Range scan"): every comparison is bit for bit against
fpyv_amd.rays.evaluate - the kernel's own lane function on the host - on the positions and attitudes read back from the batch."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import gate_course as gc
import range_scene as S
from conftest import REPO
from fpyv_amd import _lib, load_params, sticks
from fpyv_amd import rays as RY
from fpyv_amd.env import DroneBatch, FpvVecEnv, RacerBatch
from fpyv_amd.objects import Target

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NMAX = 1000


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _pose(batch):
    s = batch.state[:10, :batch.n].cpu().numpy()
    return s[0:3].T.copy(), s[6:10].T.copy()


def _expect(batch, objects, rays=None, max_range=S.MAX_RANGE):
    p, q = _pose(batch)
    return RY.evaluate(batch.range_rays if rays is None else rays, max_range, p, q, objects)


def _scattered(n, seed=2):
    rng = np.random.default_rng(seed)
    pos = np.stack([rng.uniform(-8, 8, n), rng.uniform(-8, 8, n), rng.uniform(0.5, 8, n)], 1)
    return pos, rng.uniform(-3, 3, (n, 3)), rng.uniform(-180, 180, (n, 3)) * np.array([0.3, 0.3, 1.0])


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


# ---- T1: sizes and lists ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rays", [1, 5, 32])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 129, 1000])
def test_scan_equals_the_host_function_for_every_size_and_list(n, rays):
    ray_set = RY.derive(np.random.default_rng(rays).normal(size=(rays, 3)))
    b = DroneBatch(load_params(fps=1000), n, device=DEV, range_rays=ray_set, range_max=S.MAX_RANGE)
    b.state[:, :n].copy_(torch.from_numpy(_flown_state()[:, :n]).to(DEV))
    assert np.array_equal(_bits(b.range_rays), _bits(ray_set)) and b.range_rows.shape == (rays, b.ld)
    for count in (0, 1, 4, 8):
        b.range_rows.fill_(-1.0)
        got = b.range_scan(S.world(count))
        assert got.shape == (rays, n)
        rows = b.range_rows.cpu().numpy()
        assert np.array_equal(_bits(rows[:, :n]), _bits(_expect(b, S.world(count)))), (n, rays, count)
        assert (rows[:, n:] == -1.0).all()                  # nothing is written past the last drone
    hit = b.ranges.cpu().numpy() < S.MAX_RANGE
    assert n < 64 or hit.any()


# ---- T2: the scan leaves the handle alone ---------------------------------------------------------------------------------------
def _pair(kind):
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
    a, b = cls(p, 520, device=DEV, **kw), cls(p, 520, device=DEV, range_rays=RY.fan(9, 120.0), range_max=S.MAX_RANGE, **kw)
    for x in (a, b):
        if kind == "racer":
            x.reset()
        else:
            pos, vel, ypr = _scattered(520, seed=4)
            x.reset(position=pos, velocity=vel, ypr=ypr)
        if kind == "physics":
            x.randomize_physics(7, mass=(0.8, 1.2))
    return a, b


@pytest.mark.parametrize("kind", ["plain", "physics", "gates", "noise", "reset_pose", "racer"])
def test_a_chain_with_scans_ends_where_the_chain_without_them_ends(kind):
    plain, scanned = _pair(kind)
    world = S.world(4)
    n = plain.n
    if kind == "racer":
        rng = np.random.default_rng(6)
        acts = np.concatenate([rng.uniform(-2, 2, (40, n, 3)), rng.uniform(5, 12, (40, n, 1))], -1).astype(np.float32)
    else:
        acts = sticks.ema_noise(40, range(n), seed=8)
    a = torch.from_numpy(acts).to(DEV)
    for t in range(40):
        for x in (plain, scanned):
            x.step(a[t], return_imu=False)
        got = scanned.range_scan(world).cpu().numpy()
        assert np.array_equal(_bits(got), _bits(_expect(scanned, world))), (kind, t)
    torch.cuda.synchronize()
    for name in ("state", "reward", "done", "noise_state", "gate_word"):
        x, y = getattr(plain, name, None), getattr(scanned, name, None)
        assert (x is None) == (y is None)
        if x is not None:
            assert torch.equal(x, y), (kind, name)
    assert plain.step_counter() == scanned.step_counter() == 40
    assert plain.rotation == scanned.rotation


# ---- T3: FpvVecEnv --------------------------------------------------------------------------------------------------------------
def _env(partitions=1, n=700, **kw):
    p = load_params(fps=1000).replace(init_position=np.array([0.0, 0.0, 1.0]), ceiling=1.02)
    return FpvVecEnv(p, num_envs=n, device=DEV, object_list=S.world(4), partitions=partitions, range_rays=RY.grid(4, 3, 90.0, 60.0),
                     range_max=S.MAX_RANGE, per_drone_reset_pose=True, **kw)


def _env_expect(env):
    obs = env.obs.cpu().numpy()
    return RY.evaluate(env.batch.range_rays, S.MAX_RANGE, obs[:, 0:3], obs[:, 6:10], env.object_list)


def test_env_ranges_follow_obs_through_resets_and_auto_resets():
    env = _env()
    n = env.num_envs
    pos, vel, ypr = _scattered(n, seed=9)
    pos[:, 2] = 1.0 + 0.019 * np.arange(n) / n              # just under the ceiling: lanes reset at different steps
    env.reset(position=pos, velocity=vel * 0.1, ypr=ypr)
    assert np.array_equal(_bits(env.ranges.cpu().numpy()), _bits(_env_expect(env)))
    a = torch.zeros((n, 4), device=DEV)
    a[:, 3] = 1.0                                          # full throttle: every lane reaches the ceiling and resets
    resets = 0
    for t in range(30):
        obs, reward, done, info = env.step(a)
        resets += int(done.sum())
        assert info["ranges"].data_ptr() == env.ranges.data_ptr() and env.ranges.shape == (12, n)
        assert np.array_equal(_bits(env.ranges.cpu().numpy()), _bits(_env_expect(env))), t
        # a lane that reset is back at ITS start: its ranges are those of the reset pose, like obs
        back = done.cpu().numpy()
        if back.any():
            assert np.allclose(obs.cpu().numpy()[back, 0:3], pos[back].astype(np.float32))
    assert resets > 0
    env.close()


def test_partitions_give_the_same_bits():
    one, two = _env(1), _env(2)
    assert two.partitions == 2
    n = one.num_envs
    pos, vel, ypr = _scattered(n, seed=10)
    for e in (one, two):
        e.reset(position=pos, velocity=vel, ypr=ypr)
    a = torch.from_numpy(sticks.ema_noise(20, range(n), seed=12)).to(DEV)
    for t in range(20):
        one.step(a[t])
        for k in range(two.partitions):
            lo, hi = two.partition_range(k)
            two.step_async(k, a[t, lo:hi])
        for k in range(two.partitions):
            lo, hi = two.partition_range(k)
            obs, reward, done, info = two.step_wait(k)
            assert info["ranges"].shape == (12, hi - lo)
        torch.cuda.synchronize()
        assert torch.equal(one.batch.state, two.batch.state) and torch.equal(one.ranges, two.ranges), t
    assert np.array_equal(_bits(two.ranges.cpu().numpy()), _bits(_env_expect(two)))
    one.close(); two.close()


# ---- T4: a moving target --------------------------------------------------------------------------------------------------------
def test_a_moving_target_changes_the_ranges_as_the_host_function_says():
    n = 300
    b = DroneBatch(load_params(fps=1000), n, device=DEV, range_rays=RY.fan(16, 360.0 * 15 / 16), range_max=S.MAX_RANGE)
    pos, vel, ypr = _scattered(n, seed=13)
    b.reset(position=pos, velocity=vel, ypr=ypr)
    target = Target([0.0, 0.0, 4.0], 1.5, path=dict(radius=4.0, resolution=12))
    a = torch.zeros((n, 4), device=DEV)
    seen = []
    for t in range(12):
        target.update()
        b.step(a, object_list=[target], return_imu=False)
        got = b.range_scan().cpu().numpy()                  # None: the list the step bound
        assert np.array_equal(_bits(got), _bits(_expect(b, [target]))), t
        seen.append(got)
    assert any(not np.array_equal(seen[0], s) for s in seen[1:]) and (seen[-1] < S.MAX_RANGE).any()


# ---- T5: refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals_are_by_name_and_leave_the_next_step_working():
    p = load_params(fps=1000)
    n = 130
    with pytest.raises(ValueError, match="built without range_rays="):
        DroneBatch(p, n, device=DEV).range_scan()
    half = DroneBatch(p, n, device=DEV, fp16_state=True, range_rays=RY.fan(3, 90.0))
    half.reset()
    with pytest.raises(_lib.FpvError, match="fp16 state"):
        half.range_scan()
    b = DroneBatch(p, n, device=DEV, range_rays=RY.fan(3, 90.0), range_max=S.MAX_RANGE)
    b.reset()
    L = _lib.lib()
    for field, value, what in (("ranges_ld", 128, "ranges_ld is smaller"), ("ranges_ld", b.ld + 2, "multiple of 4"), ("ray_count", 0, "ray_count"),
                               ("ray_count", 33, "ray_count"), ("max_range", -1.0, "max_range"), ("max_range", float("nan"), "max_range"),
                               ("ranges", None, "ranges is null"), ("struct_size", 16, "struct_size")):
        s = _lib.FpvRangeScan.from_buffer_copy(b._scan)
        setattr(s, field, value)
        with pytest.raises(_lib.FpvError, match=what):
            b._range_scan_raw(s)
    with pytest.raises(ValueError, match="at most 8"):
        b.range_scan([Target([k, 0, 0], 0.1) for k in range(9)])
    with pytest.raises(_lib.FpvError, match="1..32"):
        DroneBatch(p, n, device=DEV, range_rays=np.ones((33, 3)))
    a = torch.zeros((n, 4), device=DEV)
    for x in (b, half):
        x.step(a, return_imu=False)
    got = b.range_scan(S.world(4)).cpu().numpy()
    assert np.array_equal(_bits(got), _bits(_expect(b, S.world(4)))) and b.step_counter() == 1
    assert "range_rows" not in b.state_dict()               # an output: checkpoints do not carry it


# ---- T6: the example ------------------------------------------------------------------------------------------------------------
def test_the_obstacle_avoidance_example_runs():
    r = subprocess.run([sys.executable, os.path.join(REPO, "examples", "obstacle_avoidance.py"), "--drones", "256"], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "crashes" in r.stdout
