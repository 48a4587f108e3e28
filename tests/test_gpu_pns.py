"""Point and shoot on the GPU (include/fpv_abi.h "Point and shoot"): the kernel against PointAndShoot.evaluate - its own
lane function on the host - bit for bit on the poses read back from the batch, with guard words behind every output and in the row
padding; the hand-over of its outputs to the step kernel's override; the law as the action space of FpvVecEnv(pursuit=, assist=)
against the same sequence of DroneBatch calls made by hand; reset, broadcasts and refusals."""
import functools

import numpy as np
import pytest
import torch

import pursuit_task as PT
from chase_law import CHASE_TARGET, HOVER_STICKS, chase_starts
from fpyv_amd import _lib, load_params
from fpyv_amd.env import DroneBatch, FpvVecEnv, RacerBatch
from fpyv_amd.objects import Target
from fpyv_amd.pns import PointAndShoot

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NMAX = 257
PAIRS = [("world", "level"), ("world", "frontarget"), ("drone", "level"), ("drone", "frontarget")]
CENTRE = np.array([2.0, -1.0, 4.0], dtype=np.float32)
GUARD = 1.0e30


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a.view(np.uint8)


@functools.lru_cache(maxsize=None)
def _scene():
    """(position, velocity, ypr, own target, action, pixel) for NMAX drones 2..19 m around CENTRE: half of them with the nose towards
    it (seen when within max_depth), a third below tof_effective_distance, every fifth at 15..45 m/s (the thrust limit is out of
    reach), every fifth flying away from it at 9..12.5 m/s (the limit binds), drone 4 standing still; a target of its own for every
    drone near CENTRE; commands in [-0.6, 0.6]; the caller's own pixels with a NaN for every 50th drone.  Computed once; read-only."""
    rng = np.random.default_rng(21)
    i = np.arange(NMAX)
    az, rho = rng.uniform(-np.pi, np.pi, NMAX), rng.uniform(2.0, 19.0, NMAX)
    rho[4] = 6.0
    z = np.where(i % 3 == 1, rng.uniform(0.4, 1.9, NMAX), rng.uniform(2.1, 8.0, NMAX))
    pos = np.stack([CENTRE[0] + rho * np.cos(az), CENTRE[1] + rho * np.sin(az), z], 1)
    yaw = np.where(i % 2 == 0, np.rad2deg(az) + 180.0 + rng.uniform(-25, 25, NMAX), rng.uniform(-180, 180, NMAX))
    ypr = np.stack([rng.uniform(-10, 10, NMAX), rng.uniform(-10, 10, NMAX), yaw], 1)
    vel = rng.uniform(-4, 4, (NMAX, 3))
    fast = rng.normal(size=(NMAX, 3))
    fast *= (rng.uniform(15.0, 45.0, NMAX) / np.linalg.norm(fast, axis=1))[:, None]
    vel[i % 5 == 2] = fast[i % 5 == 2]
    away = pos - CENTRE
    away *= (rng.uniform(9.0, 12.5, NMAX) / np.linalg.norm(away, axis=1))[:, None]
    vel[i % 5 == 3] = away[i % 5 == 3]                                  # flying away from the target it looks at: the limit binds
    vel[4] = 0.0                                                        # |v| = 0: the defined zero-drag case
    own = CENTRE + rng.uniform(-1.0, 1.0, (NMAX, 3))
    action = rng.uniform(-0.6, 0.6, (NMAX, 4))
    pixel = rng.uniform([0, 0], [640, 480], (NMAX, 2))
    pixel[3::50] = np.nan
    return tuple(x.astype(np.float32) for x in (pos, vel, ypr, own, action, pixel))


def _batch(n, p=None, **kw):
    b = DroneBatch(p or load_params(fps=250), n, device=DEV, **kw)
    pos, vel, ypr = _scene()[:3]
    b.reset(position=pos[:n], velocity=vel[:n], ypr=ypr[:n])
    return b


def _pose(b):
    s = b.state[:10, :b.n].cpu().numpy()
    return s[0:3].T.copy(), s[3:6].T.copy(), s[6:10].T.copy()


def _guarded(count, dtype=torch.float32, pad=16):
    return torch.full((count + pad,), GUARD if dtype == torch.float32 else 0x5A, dtype=dtype, device=DEV)


def _rows(rows, n, ld, fill):
    """[rows, ld] device rows: `fill` ([rows, n] or a scalar) in the columns of the drones, guard words in the padding"""
    t = torch.full((rows, ld), GUARD, dtype=torch.float32, device=DEV)
    t[:, :n] = torch.as_tensor(fill, dtype=torch.float32, device=DEV)
    return t


# (pixel source, commands given, every optional output, restart mask on the second call)
VARIANTS = [("shared", True, True, True), ("rows", False, False, False), ("rows", True, True, False), ("pixel", True, False, True),
            ("pixel", False, True, False)]


# ---- T1: bit identity with the host function ------------------------------------------------------------------------------------
@pytest.mark.parametrize("frame,mode", PAIRS)
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_kernel_equals_the_host_function_bit_for_bit(n, frame, mode):
    params = load_params(fps=250)
    b = _batch(n, params)
    G = PointAndShoot(params, ref_frame=frame, mode=mode)
    p, v, q = _pose(b)
    _, _, _, own, action, pixel = (x[:n] for x in _scene())
    ld = n + 12
    for source, commands, optional, restarts in VARIANTS:
        pid = _rows(4, n, ld, np.array([[0.0], [0.0], [0.0], [1.0]], dtype=np.float32).repeat(n, 1))      # a freshly reset PID
        prev = _rows(2, n, ld, float("nan"))
        host_pid, host_prev = pid[:, :n].cpu().numpy(), prev[:, :n].cpu().numpy()
        tgt_rows = _rows(3, n, ld, own.T.copy())
        dev_pixel, dev_action = torch.from_numpy(pixel.copy()).to(DEV), torch.from_numpy(action.copy()).to(DEV)
        for call in range(2):                                           # the first-call branches, then the steady ones
            rot, thrust = _guarded(9 * n), _guarded(n)
            vel, lim, vis, thr = _guarded(2 * n), _guarded(n, torch.uint8), _guarded(n, torch.uint8), _guarded(n)
            s = G.derive()
            s.pid_state, s.pid_ld, s.prev_pixel, s.prev_pixel_ld = pid.data_ptr(), ld, prev.data_ptr(), ld
            s.rotation, s.thrust = rot.data_ptr(), thrust.data_ptr()
            if optional:
                s.pixel_velocity, s.limited, s.visible, s.throttle = vel.data_ptr(), lim.data_ptr(), vis.data_ptr(), thr.data_ptr()
            kw = {}
            if source == "shared":
                s.target, kw["target"] = CENTRE.ctypes.data, CENTRE
            elif source == "rows":
                s.target_rows, s.target_ld, kw["target"] = tgt_rows.data_ptr(), ld, np.ascontiguousarray(own.T)
            else:
                s.pixel, kw["pixel"] = dev_pixel.data_ptr(), pixel
            if commands:
                s.action, kw["action"] = dev_action.data_ptr(), action
            mask = dev_mask = None
            if restarts and call == 1:
                mask = (np.arange(n) % 3 == 0).astype(np.uint8)
                dev_mask = torch.from_numpy(mask).to(DEV)
                s.restart, kw["restart"] = dev_mask.data_ptr(), mask
            b._sensor_raw(b._L.fpv_pns_guide, s, None)
            torch.cuda.synchronize()
            w = G.evaluate(p, v, q, pid_state=host_pid, prev_pixel=host_prev, **kw)
            host_pid, host_prev = w["pid_state"], w["prev_pixel"]
            tag = (n, frame, mode, source, commands, optional, call)
            assert np.array_equal(_bits(rot[:9 * n].cpu().numpy()), _bits(w["rotation"].reshape(-1))), tag
            assert np.array_equal(_bits(thrust[:n].cpu().numpy()), _bits(w["thrust"])), tag
            assert np.array_equal(_bits(pid[:, :n].cpu().numpy()), _bits(host_pid)), tag
            assert np.array_equal(_bits(prev[:, :n].cpu().numpy()), _bits(host_prev)), tag
            used = dict(vel=2 * n, lim=n, vis=n, thr=n) if optional else dict(vel=0, lim=0, vis=0, thr=0)
            if optional:
                assert np.array_equal(_bits(vel[:2 * n].cpu().numpy()), _bits(w["pixel_velocity"].reshape(-1))), tag
                assert np.array_equal(_bits(thr[:n].cpu().numpy()), _bits(w["throttle"])), tag
                assert np.array_equal(lim[:n].cpu().numpy(), w["limited"]) and np.array_equal(vis[:n].cpu().numpy(), w["visible"].astype(np.uint8)), tag
            # nothing past the last drone of any output (nothing at all in an output that was not given), nothing in the row padding
            for t, k in ((rot, 9 * n), (thrust, n), (vel, used["vel"]), (thr, used["thr"])):
                assert bool((t[k:] == GUARD).all()), tag
            assert bool((lim[used["lim"]:] == 0x5A).all()) and bool((vis[used["vis"]:] == 0x5A).all()), tag
            for t in (pid, prev, tgt_rows):
                assert bool((t[:, n:] == GUARD).all()), tag
            seen = np.isfinite(w["thrust"])
            assert np.all(host_pid[3, seen] == 0.0) and np.all(np.isfinite(host_prev[:, seen]))
            if mask is not None:                                        # a restarted lane: its first call again
                again = seen & (mask != 0)
                assert np.all(host_pid[1, again] == 0.0)                # no derivative on a PID's first call
                if optional:
                    assert np.all(w["pixel_velocity"][again] == 0.0) and (n < 60 or again.sum() >= 5)
            if n == NMAX and source == "shared" and call == 0:
                # the lane set: unseen and seen, not limited, limited and out of reach, below tof, standing still
                lim_h = w["limited"]
                assert 40 < seen.sum() < n - 40 and seen[4] and np.all(np.isnan(w["thrust"][~seen])) and np.all(lim_h[~seen] == 0)
                assert (lim_h[seen] == 0).sum() >= 40 and (lim_h == 1).sum() >= 2 and (lim_h == 2).sum() >= 10, np.bincount(lim_h)
                assert (seen & (p[:, 2] < params.point_and_shoot["tof_effective_distance"]) & (v[:, 2] < 0)).sum() >= 10
                assert np.all(w["thrust"][lim_h == 2] == np.float32(params.max_throttle_in_force))
                assert np.all(host_pid[3, ~seen] == 1.0) and np.all(np.isnan(host_prev[:, ~seen]))


# ---- T2: the outputs go straight into the step's override -----------------------------------------------------------------------
def test_hand_over_to_the_step_equals_the_host_outputs_uploaded_as_the_override():
    params, n, steps = load_params(fps=250), 256, 200
    G = PointAndShoot(params)
    target = Target(CHASE_TARGET["position"], CHASE_TARGET["radius"], path=dict(CHASE_TARGET["path"]))
    pos, ypr = chase_starts(n)
    ypr[::4, 2] += 180.0                                               # every fourth drone looks away: never guided
    sticks = torch.from_numpy(np.tile(HOVER_STICKS.astype(np.float32), (n, 1))).to(DEV)
    command = np.random.default_rng(3).uniform(-0.3, 0.3, (n, 4)).astype(np.float32)
    dev_command = torch.from_numpy(command).to(DEV)
    dev, host = (DroneBatch(params, n, device=DEV) for _ in range(2))
    for b in (dev, host):
        b.reset(position=pos, velocity=np.zeros(3), ypr=ypr)
    host_pid = host_prev = None
    never, limited = np.ones(n, dtype=bool), 0
    for t in range(steps):
        target.update()
        rot, thrust = dev.point_and_shoot(None, dev_command, target=target)
        assert rot.shape == (n, 3, 3) and thrust.shape == (n,) and rot.data_ptr() == dev._pns_out["rotation"].data_ptr()
        dev.step(sticks, object_list=[], rotation_matrix=rot, thrust_force=thrust, return_imu=False)
        p, v, q = (host.state[a:b, :n].t().cpu().numpy() for a, b in ((0, 3), (3, 6), (6, 10)))
        w = G.evaluate(p, v, q, action=command, target=target, pid_state=host_pid, prev_pixel=host_prev)
        host_pid, host_prev = w["pid_state"], w["prev_pixel"]
        never &= np.isnan(w["thrust"])
        limited += int((w["limited"] > 0).sum())
        host.step(sticks, object_list=[], rotation_matrix=torch.from_numpy(w["rotation"]).to(DEV), thrust_force=torch.from_numpy(w["thrust"]).to(DEV),
                  return_imu=False)
        assert torch.equal(dev.state.view(torch.int32), host.state.view(torch.int32)), t
    assert np.array_equal(_bits(dev.force_multiplier_pid.state[:, :n].cpu().numpy()), _bits(host_pid))
    assert np.array_equal(_bits(dev.pns_prev_pixel[:, :n].cpu().numpy()), _bits(host_prev))
    assert np.array_equal(_bits(dev.pixel_velocity.cpu().numpy()), _bits(w["pixel_velocity"]))
    assert np.array_equal(dev.thrust_limited.cpu().numpy(), w["limited"]) and np.array_equal(_bits(dev.pns_throttle.cpu().numpy()), _bits(w["throttle"]))
    assert 30 <= never.sum() <= n - 100
    print(f"hand-over: {n - never.sum()} drones guided, {limited} limited drone-steps")


# ---- T3: the law as the env's action space ----------------------------------------------------------------------------------------
CEIL = 10.2


def _env_scene(n, seed=8):
    """climbing starts just below the ceiling (most drones end an episode within 50 steps and auto-reset), a standing target of its
    own 6..9 m ahead of and above every drone (seen by the camera, which looks 35 degrees up)"""
    rng = np.random.default_rng(seed)
    pos = np.stack([rng.uniform(-5, 5, n), rng.uniform(-5, 5, n), rng.uniform(9.0, 10.1, n)], axis=1).astype(np.float32)
    vel = np.stack([rng.uniform(-1, 1, n), rng.uniform(-1, 1, n), rng.uniform(0.5, 8.0, n)], axis=1).astype(np.float32)
    centre = pos + np.stack([rng.uniform(6, 9, n), rng.uniform(-2, 2, n), rng.uniform(2, 5, n)], axis=1).astype(np.float32)
    return pos, vel, dict(centre=centre, radius=0.5, path_radius=0.0)


def test_env_with_assist_equals_the_same_calls_made_by_hand_and_reset_lanes_restart():
    n, steps, params = 256, 50, load_params(fps=250, ceiling=CEIL)
    pos, vel, targets = _env_scene(n)
    law = PointAndShoot(params, ref_frame="drone", mode="frontarget", max_depth=20.0)
    sticks = (0.0, 0.0, 0.0, -0.646)
    env = FpvVecEnv(params, num_envs=n, device=DEV, auto_reset=True, pursuit=PT.task(targets=targets, respawn_on_done=False), assist=law, assist_sticks=sticks)
    hand = DroneBatch(params, n, device=DEV, auto_reset=True, track_episodes=True, with_accel=False, pursuit=PT.task(targets=targets, respawn_on_done=False))
    hand.set_chase_camera(None, max_depth=20.0)
    env.reset(position=pos, velocity=vel)
    hand.reset(position=pos, velocity=vel)
    commands = torch.from_numpy(np.random.default_rng(5).uniform(-0.4, 0.4, (steps, n, 4)).astype(np.float32)).to(DEV)
    hand_sticks = torch.tensor(sticks, dtype=torch.float32, device=DEV).expand(n, 4).contiguous()
    guided = restarted = dones = 0
    was_done = torch.zeros(n, dtype=torch.bool, device=DEV)
    for t in range(steps):
        _, reward, done, info = env.step(commands[t])
        rot, thrust = hand.point_and_shoot(None, commands[t], ref_frame="drone", mode="frontarget", target=hand.target_position_rows,
                                           restart=hand.done_u8)
        hand.step(hand_sticks, rotation_matrix=rot, thrust_force=thrust, return_imu=False)
        eb = env.batch
        for name in ("state", "reward", "ep_return", "target_rows", "target_position_rows", "pns_prev_pixel"):
            assert torch.equal(getattr(eb, name).view(torch.int32), getattr(hand, name).view(torch.int32)), (t, name)
        assert torch.equal(eb.force_multiplier_pid.state.view(torch.int32), hand.force_multiplier_pid.state.view(torch.int32)), t
        assert torch.equal(done, hand.done) and torch.equal(eb._pns_out["thrust"].view(torch.int32), thrust.view(torch.int32)), t
        # a lane the previous step reset in the kernel: this call restarted it - a guided one made its first call again (no pixel
        # velocity, no derivative), one that is not guided holds a fresh PID and no prev_pixel
        seen = torch.isfinite(eb._pns_out["thrust"])
        again, idle = was_done & seen, was_done & ~seen
        assert bool((eb.pixel_velocity[again] == 0.0).all()) and bool((eb.force_multiplier_pid.state[1, :n][again] == 0.0).all()), t
        assert bool((eb.force_multiplier_pid.state[3, :n][idle] == 1.0).all()) and bool(torch.isnan(eb.pns_prev_pixel[:, :n][:, idle]).all()), t
        moving = seen & ~was_done
        if t > 0:
            assert bool((eb.pixel_velocity[moving] != 0.0).any()), t
        guided += int(seen.sum())
        restarted += int(again.sum())
        dones += int(done.sum())
        was_done = done.clone()
    assert dones >= 20 and guided >= 50 * 20 and restarted >= 1, (dones, guided, restarted)
    # reset(mask) clears the law's rows of exactly the masked drones; the checkpoint carries them
    mask = torch.zeros(n, dtype=torch.bool, device=DEV)
    mask[::3] = True
    before_pid, before_prev = env.batch.force_multiplier_pid.state[:, :n].clone(), env.batch.pns_prev_pixel[:, :n].clone()
    assert int((mask & torch.isfinite(before_prev[0])).sum()) > 5
    env.reset(mask)
    after_pid, after_prev = env.batch.force_multiplier_pid.state[:, :n], env.batch.pns_prev_pixel[:, :n]
    assert bool(torch.isnan(after_prev[:, mask]).all()) and bool((after_pid[:3, mask] == 0.0).all()) and bool((after_pid[3, mask] == 1.0).all())
    assert torch.equal(after_prev[:, ~mask].view(torch.int32), before_prev[:, ~mask].view(torch.int32))
    assert torch.equal(after_pid[:, ~mask].view(torch.int32), before_pid[:, ~mask].view(torch.int32))
    d = env.state_dict()
    assert d["pns_prev_pixel"].shape == (2, n) and d["pns_pid_rows"].shape == (4, n) and d["pns_target_rows"].shape == (3, n)
    other = FpvVecEnv(params, num_envs=n, device=DEV, auto_reset=True, pursuit=PT.task(targets=targets, respawn_on_done=False), assist=law, assist_sticks=sticks)
    other.load_state_dict(d)
    env.step(commands[0]); other.step(commands[0])
    for name in ("state", "pns_prev_pixel", "target_rows"):
        assert torch.equal(getattr(env.batch, name).view(torch.int32), getattr(other.batch, name).view(torch.int32)), name
    assert torch.equal(env.batch.force_multiplier_pid.state.view(torch.int32), other.batch.force_multiplier_pid.state.view(torch.int32))
    # the three refusals
    with pytest.raises(ValueError, match="assist= needs pursuit="):
        FpvVecEnv(params, num_envs=8, device=DEV, assist=law)
    with pytest.raises(ValueError, match="guided=True"):
        FpvVecEnv(params, num_envs=8, device=DEV, pursuit=PT.task(guide=dict(max_depth=40.0)), guided=True, assist=law)
    with pytest.raises(ValueError, match="partitions > 1"):
        FpvVecEnv(params, num_envs=256, device=DEV, pursuit=PT.task(), partitions=2, assist=law)
    for e in (env, other):
        e.close()


# ---- T4: broadcasts, reset, refusals -----------------------------------------------------------------------------------------------
def test_broadcast_inputs_reset_mask_and_racer_and_fp16_handles_are_refused_by_name():
    params, n = load_params(fps=250), 130
    b = _batch(n, params)
    p, v, q = _pose(b)
    rot, thrust = b.point_and_shoot([320.0, 200.0], [0.1, -0.2, 0.05, 0.1], ref_frame="drone", mode="frontarget")
    torch.cuda.synchronize()
    w = PointAndShoot(params, ref_frame="drone", mode="frontarget").evaluate(p, v, q, pixel=np.tile([320.0, 200.0], (n, 1)), action=[0.1, -0.2, 0.05, 0.1])
    assert np.array_equal(_bits(rot.cpu().numpy()), _bits(w["rotation"])) and np.array_equal(_bits(thrust.cpu().numpy()), _bits(w["thrust"]))
    assert bool(torch.isfinite(thrust).all()) and b.thrust_limited.shape == (n,) and b.pixel_velocity.shape == (n, 2)
    # a second call, action None = zeros, against a shared Target: then reset(mask)
    b.point_and_shoot(None, None, target=Target(CENTRE, 0.5))
    before = b.pns_prev_pixel[:, :n].clone()
    mask = torch.zeros(n, dtype=torch.bool, device=DEV)
    mask[::3] = True
    b.reset(mask=mask)
    after = b.pns_prev_pixel[:, :n]
    assert bool(torch.isnan(after[:, mask]).all()) and torch.equal(after[:, ~mask].view(torch.int32), before[:, ~mask].view(torch.int32))
    assert bool((b.force_multiplier_pid.state[3, :n][mask] == 1.0).all())
    with pytest.raises(ValueError, match="pixel=None needs target="):
        b.point_and_shoot(None, None)
    with pytest.raises(ValueError, match="Unknown mode"):
        b.point_and_shoot([1.0, 2.0], None, mode="sideways")
    with pytest.raises(ValueError, match="action must be"):
        b.point_and_shoot([1.0, 2.0], [0.0, 0.0, 0.0])
    with pytest.raises(_lib.FpvError, match="Racer handle"):
        RacerBatch(None, 8, device=DEV).point_and_shoot([320.0, 240.0], None)
    with pytest.raises(_lib.FpvError, match="fp16 state"):
        DroneBatch(params, 8, device=DEV, fp16_state=True).point_and_shoot([320.0, 240.0], None)
