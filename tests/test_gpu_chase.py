"""The target chase on the GPU (include/fpv_abi.h "Target chase"): the kernel against ChaseGuidance.evaluate - its own lane
function on the host - bit for bit on the poses read back from the batch; the hand-over of its outputs to the step kernel's override;
the closed loop; and the reset of the guidance PID."""
import functools

import numpy as np
import pytest
import torch

from chase_law import CHASE_TARGET, HOVER_STICKS, chase_starts
from fpyv_amd import _lib, load_params
from fpyv_amd.chase import ChaseGuidance
from fpyv_amd.env import DroneBatch, RacerBatch
from fpyv_amd.objects import Target

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NMAX = 257
PAIRS = [("world", "level"), ("world", "frontarget"), ("drone", "level"), ("drone", "frontarget")]
TARGET = (np.array([2.0, -1.0, 4.0], dtype=np.float32), 0.5)
GUARD = 1.0e30


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a.view(np.uint8)


@functools.lru_cache(maxsize=None)
def _scene():
    """(position, velocity, ypr) [NMAX, 3]: drones 2..19 m around the target, half of them with the nose towards it (seen when within
    max_depth), a third below tof_effective_distance, a part of the seen ones beyond the UWB range.  Computed once; read-only."""
    rng = np.random.default_rng(11)
    az, rho = rng.uniform(-np.pi, np.pi, NMAX), rng.uniform(2.0, 19.0, NMAX)
    rho[4] = 6.0                                                        # drone 4 sees the target, standing still (below)
    z = np.where(np.arange(NMAX) % 3 == 1, rng.uniform(0.4, 1.9, NMAX), rng.uniform(2.1, 8.0, NMAX))
    pos = np.stack([TARGET[0][0] + rho * np.cos(az), TARGET[0][1] + rho * np.sin(az), z], 1)
    yaw = np.where(np.arange(NMAX) % 2 == 0, np.rad2deg(az) + 180.0 + rng.uniform(-25, 25, NMAX), rng.uniform(-180, 180, NMAX))
    ypr = np.stack([rng.uniform(-10, 10, NMAX), rng.uniform(-10, 10, NMAX), yaw], 1)
    vel = rng.uniform(-4, 4, (NMAX, 3))
    vel[4] = 0.0                                                        # |v| = 0: the defined zero-drag case
    return pos.astype(np.float32), vel.astype(np.float32), ypr.astype(np.float32)


def _batch(n, p=None, **kw):
    b = DroneBatch(p or load_params(fps=250), n, device=DEV, **kw)
    pos, vel, ypr = _scene()
    b.reset(position=pos[:n], velocity=vel[:n], ypr=ypr[:n])
    return b


def _pose(b):
    s = b.state[:10, :b.n].cpu().numpy()
    return s[0:3].T.copy(), s[3:6].T.copy(), s[6:10].T.copy()


def _guarded(count, dtype=torch.float32, pad=16):
    t = torch.full((count + pad,), GUARD if dtype == torch.float32 else 0x5A, dtype=dtype, device=DEV)
    return t


# ---- T1: bit identity with the host function ------------------------------------------------------------------------------------
@pytest.mark.parametrize("frame,mode", PAIRS)
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_kernel_equals_the_host_function_bit_for_bit(n, frame, mode):
    params = load_params(fps=250)
    b = _batch(n, params)
    G = ChaseGuidance(params, ref_frame=frame, mode=mode)
    p, v, q = _pose(b)
    ld = n + 12                                                         # the padding of the PID rows carries guard words
    rows = torch.full((4, ld), GUARD, dtype=torch.float32, device=DEV)
    rows[:, :n] = 0.0
    rows[3, :n] = 1.0                                                   # a freshly reset PID
    host_rows = rows[:, :n].cpu().numpy()
    given = None
    for with_pixel in (False, True):
        for call in range(2):                                           # the PID's first-call branch, then its steady branch
            rot, thrust, pix, vis = _guarded(9 * n), _guarded(n), _guarded(2 * n), _guarded(n, torch.uint8)
            s = G.derive(TARGET)
            s.pid_state, s.pid_ld = rows.data_ptr(), ld
            s.rotation, s.thrust, s.pixel_out, s.visible = rot.data_ptr(), thrust.data_ptr(), pix.data_ptr(), vis.data_ptr()
            dev_pixel = None
            if with_pixel:
                dev_pixel = torch.from_numpy(given).to(DEV)
                s.pixel = dev_pixel.data_ptr()
            b._sensor_raw(b._L.fpv_chase_guide, s, None)
            torch.cuda.synchronize()
            w_rot, w_thrust, w_pix, w_vis, host_rows = G.evaluate(p, v, q, TARGET, host_rows, given if with_pixel else None)
            tag = (n, frame, mode, with_pixel, call)
            assert np.array_equal(_bits(rot[:9 * n].cpu().numpy()), _bits(w_rot.reshape(-1))), tag
            assert np.array_equal(_bits(thrust[:n].cpu().numpy()), _bits(w_thrust)), tag
            assert np.array_equal(_bits(pix[:2 * n].cpu().numpy()), _bits(w_pix.reshape(-1))), tag
            assert np.array_equal(vis[:n].cpu().numpy(), w_vis.astype(np.uint8)), tag
            assert np.array_equal(_bits(rows[:, :n].cpu().numpy()), _bits(host_rows)), tag
            # nothing past the last drone of any output, nothing in the padding of the PID rows
            for t, used in ((rot, 9 * n), (thrust, n), (pix, 2 * n)):
                assert bool((t[used:] == GUARD).all()), tag
            assert bool((vis[n:] == 0x5A).all()) and bool((rows[:, n:] == GUARD).all()), tag
            if not with_pixel and call == 1:
                # the caller's own pixels for the second pass: what the kernel found, moved a little, NaN where it found nothing,
                # and NaN for two drones that do see the target
                given = w_pix.copy()
                given[np.isfinite(given[:, 0])] += np.float32(1.25)
                given[3::50] = np.nan
            if n == NMAX and not with_pixel and call == 0:
                far = np.linalg.norm(p - TARGET[0], axis=1) - TARGET[1] > params.UWB_sensor_max_range
                low = p[:, 2] < params.point_and_shoot["tof_effective_distance"]
                assert 40 < w_vis.sum() < n - 40 and (w_vis & far).sum() >= 3 and (w_vis & low).sum() >= 10 and w_vis[4]
                assert np.all(np.isnan(w_thrust[~w_vis])) and np.all(np.isfinite(w_thrust[w_vis]))
                assert np.all(host_rows[3, w_vis] == 0.0) and np.all(host_rows[3, ~w_vis] == 1.0)


# ---- T2: the outputs go straight into the step's override -----------------------------------------------------------------------
def test_hand_over_to_the_step_equals_the_host_outputs_uploaded_as_the_override():
    params, n, steps = load_params(fps=250), 256, 50
    G = ChaseGuidance(params)
    target = Target(CHASE_TARGET["position"], CHASE_TARGET["radius"], path=dict(CHASE_TARGET["path"]))
    pos, ypr = chase_starts(n)
    ypr[::4, 2] += 180.0                                               # every fourth drone looks away: never guided
    sticks = torch.from_numpy(np.tile(HOVER_STICKS.astype(np.float32), (n, 1))).to(DEV)
    dev, host, plain = (DroneBatch(params, n, device=DEV) for _ in range(3))
    for b in (dev, host, plain):
        b.reset(position=pos, velocity=np.zeros(3), ypr=ypr)
    host_rows, never = None, np.ones(n, dtype=bool)
    for _ in range(steps):
        target.update()
        rot, thrust = dev.calculate_needed_force_orientation(None, target)
        assert rot.shape == (n, 3, 3) and thrust.shape == (n,) and rot.data_ptr() == dev._chase_out[0].data_ptr()
        dev.step(sticks, object_list=[], rotation_matrix=rot, thrust_force=thrust, return_imu=False)
        p, v, q = (x for x in (host.state[0:3, :n].t().cpu().numpy(), host.state[3:6, :n].t().cpu().numpy(), host.state[6:10, :n].t().cpu().numpy()))
        w_rot, w_thrust, _, w_vis, host_rows = G.evaluate(p, v, q, target, host_rows)
        never &= np.isnan(w_thrust)
        host.step(sticks, object_list=[], rotation_matrix=torch.from_numpy(w_rot).to(DEV), thrust_force=torch.from_numpy(w_thrust).to(DEV),
                  return_imu=False)
        plain.step(sticks, object_list=[], return_imu=False)
    torch.cuda.synchronize()
    assert torch.equal(dev.state.view(torch.int32), host.state.view(torch.int32))
    assert np.array_equal(_bits(dev.force_multiplier_pid.state[:, :n].cpu().numpy()), _bits(host_rows))
    assert 30 <= never.sum() <= n - 100
    idx = torch.from_numpy(np.flatnonzero(never)).to(DEV)
    assert torch.equal(dev.state[:, idx].view(torch.int32), plain.state[:, idx].view(torch.int32))
    idx = torch.from_numpy(np.flatnonzero(~never)).to(DEV)
    assert not torch.equal(dev.state[:, idx].view(torch.int32), plain.state[:, idx].view(torch.int32))


# ---- T3: the chase works ----------------------------------------------------------------------------------------------------------
def test_guided_drones_come_closer_to_a_moving_target_than_drones_on_their_hover_sticks():
    """a property, not parity: the scenario tests/test_chase_host.py flies in float64 on the CPU first"""
    params, n, steps = load_params(fps=250), 256, 600
    pos, ypr = chase_starts(n)
    sticks = torch.from_numpy(np.tile(HOVER_STICKS.astype(np.float32), (n, 1))).to(DEV)
    closest = {}
    for guided in (True, False):
        target = Target(CHASE_TARGET["position"], CHASE_TARGET["radius"], path=dict(CHASE_TARGET["path"]))
        b = DroneBatch(params, n, device=DEV)
        b.reset(position=pos, velocity=np.zeros(3), ypr=ypr)
        best = torch.full((n,), float("inf"), device=DEV)
        for _ in range(steps):
            target.update()
            c = torch.as_tensor(np.asarray(target.position, dtype=np.float32), device=DEV)
            best = torch.minimum(best, (b.position - c).norm(dim=1))
            if guided:
                rot, thrust = b.calculate_needed_force_orientation(None, target)
                b.step(sticks, object_list=[], rotation_matrix=rot, thrust_force=thrust, return_imu=False)
            else:
                b.step(sticks, object_list=[], return_imu=False)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(b.state[:, :n]).all())
        closest[guided] = float(best.median())
    print(f"median closest approach: guided {closest[True]:.2f} m, hover sticks {closest[False]:.2f} m")
    assert closest[True] < closest[False]


# ---- T4: reset, track, refusals -----------------------------------------------------------------------------------------------------
def test_reset_with_a_mask_clears_the_chase_pid_of_exactly_the_masked_drones():
    n = 130
    b = _batch(n)
    for _ in range(3):
        b.calculate_needed_force_orientation(None, TARGET)
    before = b.force_multiplier_pid.state[:, :n].clone()
    guided = before[3] == 0.0
    assert 20 < int(guided.sum()) < n and bool((before[2, guided] != 0.0).all())
    mask = torch.zeros(n, dtype=torch.bool, device=DEV)
    mask[::3] = True
    b.reset(mask=mask)
    after = b.force_multiplier_pid.state[:, :n]
    assert int((mask & guided).sum()) > 5
    assert bool((after[:3, mask] == 0.0).all()) and bool((after[3, mask] == 1.0).all())
    assert torch.equal(after[:, ~mask].view(torch.int32), before[:, ~mask].view(torch.int32))


def test_track_gives_the_pixel_alone_and_racer_and_fp16_handles_are_refused_by_name():
    params, n = load_params(fps=250), 65
    b = _batch(n, params)
    rows = b.force_multiplier_pid.state.clone()
    pix, vis = b.track(TARGET)
    torch.cuda.synchronize()
    p, v, q = _pose(b)
    _, _, w_pix, w_vis, _ = ChaseGuidance(params).evaluate(p, v, q, TARGET)
    assert pix.shape == (n, 2) and vis.dtype == torch.bool
    assert np.array_equal(_bits(pix.cpu().numpy()), _bits(w_pix)) and np.array_equal(vis.cpu().numpy(), w_vis)
    assert torch.equal(b.force_multiplier_pid.state.view(torch.int32), rows.view(torch.int32))       # no PID was advanced
    # the caller's own pixel, broadcast from [2]
    rot, thrust = b.calculate_needed_force_orientation([320.0, 240.0], TARGET, ref_frame="drone", mode="frontarget")
    assert bool(torch.isfinite(thrust).all()) and bool(torch.isfinite(rot).all())
    with pytest.raises(_lib.FpvError, match="Racer handle"):
        RacerBatch(None, 8, device=DEV).calculate_needed_force_orientation(None, TARGET)
    with pytest.raises(_lib.FpvError, match="fp16 state"):
        DroneBatch(params, 8, device=DEV, fp16_state=True).calculate_needed_force_orientation(None, TARGET)
    with pytest.raises(ValueError, match="Unknown mode"):
        b.calculate_needed_force_orientation(None, TARGET, mode="sideways")
