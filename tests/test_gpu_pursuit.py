"""The pursuit task on the GPU (include/fpv_abi.h "Pursuit task"): the kernel against PursuitTask.evaluate - its own lane
function on the host - bit for bit over the seeded scene of tests/pursuit_task.py, with and without the guidance law; the reset call
and its mask; the task inside FpvVecEnv (reward hand-over, episode returns, partitions); the closed loop; and the old paths, which
a batch without pursuit= must leave exactly as they were."""
import ctypes as C

import numpy as np
import pytest
import torch

import pursuit_task as PT
from fpyv_amd import _lib, load_params
from fpyv_amd.env import DroneBatch, FpvVecEnv, RacerBatch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 1.0e30
CALLS = 12


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a.view(np.uint8)


def _same(dev, host):
    return np.array_equal(_bits(dev.cpu().numpy() if torch.is_tensor(dev) else dev), _bits(np.asarray(host)))


def _f32(shape):
    return torch.full(shape, GUARD, dtype=torch.float32, device=DEV)


def _u8(count):
    return torch.full((count,), 0x5A, dtype=torch.uint8, device=DEV)


class Rig:
    """A plain batch of n drones and caller-owned, guard-filled buffers for everything a pursuit call reads and writes: rows with
    ld = n + 12, outputs with 16 cells of padding.  `call` uploads a pose, launches and returns what the device holds."""

    def __init__(self, n, guide, params):
        self.n, self.ld, self.params = n, n + 12, params
        self.task = PT.task(targets=PT.start_targets(n), guide=dict(max_depth=40.0) if guide else None)
        self.b = DroneBatch(params, n, device=DEV)
        self.b.reset()
        ld = self.ld
        self.rows, self.obs, self.pos = _f32((8, ld)), _f32((7, ld)), _f32((3, ld))
        self.rows.view(torch.int32)[:, :n] = torch.from_numpy(self.task.rows(n)[:, :n].view(np.int32).copy()).to(DEV)
        self.event, self.done = _u8(n + 16), _u8(n + 16)
        self.paid, self.reward, self.ep = _f32((n + 16,)), _f32((n + 16,)), _f32((n + 16,))
        self.circle = torch.from_numpy(self.task.circle).to(DEV)
        s = self.s = self.task.derive(PT.DT)
        s.targets, s.targets_ld, s.circle = self.rows.data_ptr(), ld, self.circle.data_ptr()
        s.obs, s.obs_ld, s.position, s.position_ld = self.obs.data_ptr(), ld, self.pos.data_ptr(), ld
        s.event, s.reward_out = self.event.data_ptr(), self.paid.data_ptr()
        self.pid = self.rot = self.thrust = self.pix = self.vis = None
        if guide:
            self.pid, self.rot, self.thrust, self.pix, self.vis = _f32((4, ld)), _f32((9 * n + 16,)), _f32((n + 16,)), _f32((2 * n + 16,)), _u8(n + 16)
            self.pid[:3, :n], self.pid[3, :n] = 0.0, 1.0
            g = self.g = self.task.chase(params)
            g.pid_state, g.pid_ld, g.rotation, g.thrust = self.pid.data_ptr(), ld, self.rot.data_ptr(), self.thrust.data_ptr()
            g.pixel_out, g.visible = self.pix.data_ptr(), self.vis.data_ptr()
            s.guide = C.pointer(g)
        self.buf = _lib.FpvBuffers.from_buffer_copy(self.b._buf)
        self.buf.reward, self.buf.done, self.buf.ep_return = self.reward.data_ptr(), self.done.data_ptr(), self.ep.data_ptr()

    def call(self, p, v, q, flags, step_reward, ep_return, reset):
        n, b = self.n, self.b
        b.state[:10, :n] = torch.from_numpy(np.concatenate([p.T, v.T, q.T]).astype(np.float32)).to(DEV)
        self.reward[:n], self.ep[:n] = torch.from_numpy(step_reward).to(DEV), torch.from_numpy(ep_return).to(DEV)
        mask = None
        if reset:
            mask = None if flags is None else torch.from_numpy(flags.astype(np.uint8)).to(DEV)
            rc = b._L.fpv_pursuit_reset(b._handle, C.byref(self.buf), C.byref(self.s), mask.data_ptr() if mask is not None else None, b._stream())
        else:
            self.done[:n] = torch.from_numpy(flags.astype(np.uint8)).to(DEV)
            rc = b._L.fpv_pursuit_step(b._handle, C.byref(self.buf), C.byref(self.s), b._stream())
        _lib.check(rc)
        torch.cuda.synchronize()
        s = b.state[:10, :n].cpu().numpy()                     # the poses the kernel read, back from the batch
        return s[0:3].T.copy(), s[3:6].T.copy(), s[6:10].T.copy()

    def read(self):
        """what the device holds for the n drones, as NumPy arrays"""
        n, h = self.n, lambda t: t.cpu().numpy()  # noqa: E731
        r = dict(rows=h(self.rows[:, :n]), obs=h(self.obs[:, :n]), pos=h(self.pos[:, :n]), event=h(self.event[:n]), paid=h(self.paid[:n]),
                 reward=h(self.reward[:n]), ep=h(self.ep[:n]))
        if self.pid is not None:
            r.update(pid=h(self.pid[:, :n]), rot=h(self.rot[:9 * n]).reshape(n, 9), thrust=h(self.thrust[:n]), pix=h(self.pix[:2 * n]).reshape(n, 2),
                     vis=h(self.vis[:n]))
        return r

    def guards_hold(self):
        n, ok = self.n, True
        for t in (self.rows, self.obs, self.pos) + ((self.pid,) if self.pid is not None else ()):
            ok &= bool((t[:, n:] == GUARD).all())
        for t, used in ((self.paid, n), (self.reward, n), (self.ep, n)) + (((self.rot, 9 * n), (self.thrust, n), (self.pix, 2 * n)) if self.rot is not None else ()):
            ok &= bool((t[used:] == GUARD).all())
        for t in (self.event, self.done) + ((self.vis,) if self.vis is not None else ()):
            ok &= bool((t[n:] == 0x5A).all())
        return ok


# ---- G1: bit identity with the host function -------------------------------------------------------------------------------------
@pytest.mark.parametrize("guide", [False, True])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 129, 257])
def test_kernel_equals_the_host_function_bit_for_bit(n, guide):
    params = load_params(fps=250)
    P, V, Q, D, _ = PT.scene(n)
    rig = Rig(n, guide, params)
    rng = np.random.default_rng(n)
    host_rows, host_pid = rig.task.rows(n), None
    events = rebases = 0
    for c in range(CALLS):
        reset = c == 0
        step_reward, ep = rng.normal(size=n).astype(np.float32), rng.normal(size=n).astype(np.float32)
        p, v, q = rig.call(P[c], V[c], Q[c], D[c], step_reward, ep, reset)
        want = rig.task.evaluate(p, v, q, host_rows, PT.DT, done=D[c], reward=step_reward, reset=reset, pid_state=host_pid, params=params)
        live = D[c].astype(bool) if reset else np.ones(n, dtype=bool)       # (the reset call's mask leaves the EXACT lane out)
        got, tag = rig.read(), (n, guide, c)
        assert _same(got["rows"], want["rows"][:, :n]), tag
        assert _same(got["obs"][:, live], want["obs"][:, live]) and _same(got["pos"][:, live], want["position"][:, live]), tag
        assert _same(got["event"][live], want["event"][live]) and _same(got["paid"][live], want["paid"][live]), tag
        assert _same(got["reward"], want["reward"]), tag
        rebased = np.ones(n, dtype=bool) if reset else D[c].astype(bool)
        assert _same(got["ep"], np.where(rebased, ep, ep + want["paid"])), tag              # one fp32 addition, never on a rebasing lane
        if not live.all():                                                                    # outside the mask: every bit as it was
            assert np.all(got["obs"][:, ~live] == np.float32(GUARD)) and np.all(got["paid"][~live] == np.float32(GUARD)), tag
        if guide:
            assert _same(got["pid"], want["pid_state"]), tag
            assert _same(got["rot"][live], want["rotation"].reshape(n, 9)[live]) and _same(got["thrust"][live], want["thrust"][live]), tag
            assert _same(got["pix"][live], want["pixel"][live]) and _same(got["vis"][live], want["visible"].astype(np.uint8)[live]), tag
            host_pid = want["pid_state"]
        assert rig.guards_hold(), tag
        host_rows = want["rows"]
        events += int(want["event"].sum())
        rebases += int(D[c].sum()) if not reset else 0
    if n >= 129:
        assert events >= 20 and rebases >= 10, (events, rebases)


# ---- G2: the reset call --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("guide", [False, True])
def test_reset_with_a_mask_leaves_the_other_lanes_alone_and_a_null_mask_resets_all(guide):
    n, params = 129, load_params(fps=250)
    P, V, Q, D, _ = PT.scene(n)
    rig = Rig(n, guide, params)
    zeros = np.zeros(n, dtype=np.float32)
    host_rows, host_pid = rig.task.rows(n), None
    for c in range(4):                                  # a few calls first: rows, PID and outputs that are not their initial values
        p, v, q = rig.call(P[c], V[c], Q[c], D[c], zeros, zeros, c == 0)
        want = rig.task.evaluate(p, v, q, host_rows, PT.DT, done=D[c], reward=zeros, reset=c == 0, pid_state=host_pid, params=params)
        host_rows, host_pid = want["rows"], want.get("pid_state")
    mask = np.arange(n) % 3 == 1
    before = rig.read()
    p, v, q = rig.call(P[4], V[4], Q[4], mask, zeros, zeros, True)
    want = rig.task.evaluate(p, v, q, host_rows, PT.DT, done=mask, reward=zeros, reset=True, pid_state=host_pid, params=params)
    got = rig.read()
    for key in sorted(set(before) - {"reward", "ep"}):  # lanes outside the mask keep every bit of their rows and outputs
        lane_axis = 0 if before[key].shape[0] == n else 1
        a, b = np.take(got[key], np.flatnonzero(~mask), axis=lane_axis), np.take(before[key], np.flatnonzero(~mask), axis=lane_axis)
        assert _same(a, b), key
    assert _same(got["reward"], zeros) and _same(got["ep"], zeros)                  # (uploaded by this call) a reset call pays nothing, anywhere
    assert _same(got["rows"], want["rows"][:, :n]) and _same(got["obs"][:, mask], want["obs"][:, mask]) and _same(got["pos"][:, mask], want["position"][:, mask])
    assert not got["paid"][mask].any() and not got["event"][mask].any() and rig.guards_hold()
    assert np.all(got["rows"].view(np.uint32)[_lib.TGT_SPAWNS][mask] >> 16 == 0)
    if guide:
        assert _same(got["pid"], want["pid_state"]) and _same(got["thrust"][mask], want["thrust"][mask]) and _same(got["rot"][mask], want["rotation"].reshape(n, 9)[mask])
    # a null mask resets all
    host_rows, host_pid = want["rows"], want.get("pid_state")
    p, v, q = rig.call(P[5], V[5], Q[5], None, zeros, zeros, True)
    want = rig.task.evaluate(p, v, q, host_rows, PT.DT, done=None, reward=zeros, reset=True, pid_state=host_pid, params=params)
    got = rig.read()
    assert _same(got["rows"], want["rows"][:, :n]) and _same(got["obs"], want["obs"]) and not got["paid"].any()
    assert np.all(got["rows"].view(np.uint32)[_lib.TGT_SPAWNS] >> 16 == 0) and rig.guards_hold()
    if guide:
        assert _same(got["pid"], want["pid_state"]) and _same(got["thrust"], want["thrust"])


# ---- G3: in the env ------------------------------------------------------------------------------------------------------------------
CEIL = 10.2


def _climbing_starts(n, seed=8):
    """(position, velocity) [n, 3]: just below the ceiling and climbing, so that most drones end an episode within 30 steps (done,
    auto-reset to the params' start)"""
    rng = np.random.default_rng(seed)
    pos = np.stack([rng.uniform(-5, 5, n), rng.uniform(-5, 5, n), rng.uniform(10.0, 10.1, n)], axis=1)
    vel = np.stack([rng.uniform(-1, 1, n), rng.uniform(-1, 1, n), rng.uniform(0.5, 8.0, n)], axis=1)
    return pos.astype(np.float32), vel.astype(np.float32)


def test_in_the_env_reward_and_returns_carry_the_payment_and_partitions_change_no_bit():
    n, steps, params = 257, 30, load_params(fps=250, ceiling=CEIL)
    pos, vel = _climbing_starts(n)
    task = PT.task(targets=PT.start_targets(n))
    sticks = torch.from_numpy(np.random.default_rng(2).uniform(-0.3, 0.3, (steps, n, 4)).astype(np.float32)).to(DEV)
    kw = dict(num_envs=n, device=DEV, auto_reset=True)
    env, plain, split = FpvVecEnv(params, pursuit=task, **kw), FpvVecEnv(params, **kw), FpvVecEnv(params, pursuit=task, partitions=2, **kw)
    assert split.partitions == 2
    for e in (env, plain, split):
        e.reset(position=pos, velocity=vel)
    torch.cuda.synchronize()
    host_rows = task.rows(n)
    p, v, q = (env.batch.state[a:b, :n].t().cpu().numpy() for a, b in ((0, 3), (3, 6), (6, 10)))
    want = task.evaluate(p, v, q, host_rows, params.dt, reset=True)
    assert _same(env.batch.target_rows[:, :n], want["rows"][:, :n]) and _same(env.target_obs.t(), want["obs"])
    ep, last = np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.float32)
    dones = captures = 0
    for t in range(steps):
        _, reward, done, info = env.step(sticks[t])
        plain.step(sticks[t])
        for k in range(split.partitions):
            lo, hi = split.partition_range(k)
            split.step_async(k, sticks[t, lo:hi])
        for k in range(split.partitions):
            split.step_wait(k)
        torch.cuda.synchronize()
        assert torch.equal(env.batch.state.view(torch.int32), plain.batch.state.view(torch.int32))        # the task moves no drone
        d = done.cpu().numpy()
        assert np.array_equal(d, plain.batch.done.cpu().numpy())
        p, v, q = (env.batch.state[a:b, :n].t().cpu().numpy() for a, b in ((0, 3), (3, 6), (6, 10)))
        step_reward = plain.batch.reward.cpu().numpy()
        want = task.evaluate(p, v, q, want["rows"], params.dt, done=d, reward=step_reward)
        assert _same(reward, np.where(d, step_reward, step_reward + want["paid"])), t
        assert _same(env.batch.pursuit_reward, want["paid"]) and _same(env.batch.target_rows[:, :n], want["rows"][:, :n]), t
        assert _same(info["target_obs"].t(), want["obs"]) and _same(info["target_event"], want["event"]), t
        assert np.array_equal(info["captures"].cpu().numpy(), want["rows"].view(np.uint32)[_lib.TGT_SPAWNS, :n] >> 16), t
        # the step kernel: ep += its reward, a done lane hands it to last_return and restarts; then the task's payment, never on a done lane
        ep = ep + step_reward
        last = np.where(d, ep, last)
        ep = np.where(d, np.float32(0.0), ep + want["paid"]).astype(np.float32)
        assert _same(env.batch.ep_return, ep) and _same(env.batch.last_return, last), t
        dones += int(d.sum())
        captures += int(want["event"].sum())
    assert dones >= 5, dones
    for name in ("state", "reward", "ep_return", "last_return", "target_rows", "target_obs_rows", "target_position_rows", "pursuit_reward"):
        a, b = getattr(env.batch, name), getattr(split.batch, name)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), name
    assert torch.equal(env.batch.target_event_u8, split.batch.target_event_u8) and torch.equal(env.batch.done, split.batch.done)
    # the checkpoint carries the target rows
    other = FpvVecEnv(params, pursuit=PT.task(targets=PT.start_targets(n)), **kw)
    other.load_state_dict(env.state_dict())
    assert torch.equal(other.batch.target_rows[:, :n].view(torch.int32), env.batch.target_rows[:, :n].view(torch.int32))
    for e in (env, plain, split, other):
        e.close()


# ---- G4: the closed loop ---------------------------------------------------------------------------------------------------------------
def test_guided_env_closes_in_on_every_seen_target_and_captures():
    """the scenario tests/test_pursuit_host.py flies on the CPU first: 64 drones, each with a target of its own 8 m away; the first 16
    see it.  guided=True feeds every pursuit call's rotation / thrust to the next step.  Every drone that sees its target captures
    it or ends nearer to it than it started; at least one captures; the drones that look away are never guided."""
    params, n, seen = load_params(fps=PT.LOOP_FPS), PT.LOOP_N, PT.LOOP_SEEN
    targets, pos, ypr = PT.loop_scene()
    task = PT.task(targets=targets, **PT.LOOP_TASK_KW)
    env = FpvVecEnv(params, num_envs=n, device=DEV, auto_reset=False, pursuit=task, guided=True)
    env.reset(position=pos, velocity=np.zeros(3), ypr=ypr)
    rot, thrust = env.batch.pursuit_guidance
    start = env.target_obs[:, 6].clone()
    assert bool(((start - 8.0).abs() < 1e-3).all()) and bool(torch.isfinite(thrust[:seen]).all()) and bool(torch.isnan(thrust[seen:]).all())
    sticks = torch.from_numpy(np.tile(PT.HOVER_STICKS.astype(np.float32), (n, 1))).to(DEV)
    captured = torch.zeros(n, dtype=torch.bool, device=DEV)
    for _ in range(PT.LOOP_STEPS):
        _, _, _, info = env.step(sticks)
        captured |= info["target_event"].bool()
    torch.cuda.synchronize()
    end = env.target_obs[:, 6]
    assert bool(torch.isfinite(env.batch.state[:, :n]).all())
    print(f"{int(captured[:seen].sum())} of {seen} captured; the others end at {end[:seen][~captured[:seen]].cpu().numpy().round(2)} m")
    assert int(captured[:seen].sum()) >= 1 and bool((captured[:seen] | (end[:seen] < start[:seen])).all())
    assert torch.equal(env.captures[:seen] > 0, captured[:seen])                     # the episode's count saw every capture
    with pytest.raises(ValueError, match="guided=True needs"):
        FpvVecEnv(params, num_envs=8, device=DEV, guided=True)
    env.close()


# ---- G5: old paths unchanged; refusals that need a handle ---------------------------------------------------------------------------
def test_a_batch_without_pursuit_allocates_and_launches_nothing_new_and_keeps_its_bits():
    n, params = 130, load_params(fps=250, ceiling=CEIL)
    pos, vel = _climbing_starts(n)
    old, new = DroneBatch(params, n, device=DEV), DroneBatch(params, n, device=DEV, pursuit=None)
    sticks = torch.from_numpy(np.random.default_rng(4).uniform(-0.5, 0.5, (n, 4)).astype(np.float32)).to(DEV)
    for b in (old, new):
        b.reset(position=pos, velocity=vel)
        b.step(sticks, return_imu=False)
    torch.cuda.synchronize()
    assert torch.equal(old.state.view(torch.int32), new.state.view(torch.int32)) and torch.equal(old.reward.view(torch.int32), new.reward.view(torch.int32))
    mask = torch.arange(n, device=DEV) % 2 == 0
    for b in (old, new):
        b.reset(mask=mask)
    torch.cuda.synchronize()
    assert torch.equal(old.state.view(torch.int32), new.state.view(torch.int32))
    for name in ("target_rows", "target_obs_rows", "target_position_rows", "target_event_u8", "pursuit_reward", "pursuit_pid_rows", "pursuit_guidance", "_pursuit"):
        assert getattr(new, name) is None, name
    assert new.target_obs is None and new.captures is None
    # a batch WITH the task steps its drones exactly as the one without
    task = PT.task(targets=PT.start_targets(n))
    with_task = DroneBatch(params, n, device=DEV, pursuit=task)
    with_task.reset(position=pos, velocity=vel)
    with_task.step(sticks, return_imu=False)
    with_task.reset(mask=mask)
    torch.cuda.synchronize()
    assert torch.equal(old.state.view(torch.int32), with_task.state.view(torch.int32))
    with pytest.raises(ValueError, match="without pursuit="):
        new.set_targets([])


def test_racer_and_fp16_handles_are_refused_by_name_and_set_targets_restarts_the_distance():
    params = load_params(fps=250)
    task = PT.task(targets=PT.start_targets(8))
    with pytest.raises(_lib.FpvError, match="Racer handle"):
        RacerBatch(None, 8, device=DEV, pursuit=task).reset()
    with pytest.raises(_lib.FpvError, match="fp16 state"):
        DroneBatch(params, 8, device=DEV, fp16_state=True, pursuit=task).reset()
    n = 65
    b = DroneBatch(params, n, device=DEV, pursuit=PT.task(targets=PT.start_targets(n)))
    b.reset()
    before = b.target_rows.clone()
    mask = torch.arange(n, device=DEV) % 5 == 0
    b.set_targets(dict(centre=[1.0, 2.0, 9.0], radius=0.5, path_radius=0.0), mask=mask)
    torch.cuda.synchronize()
    rows = b.target_rows[:, :n]
    assert torch.equal(rows[:, ~mask].view(torch.int32), before[:, :n][:, ~mask].view(torch.int32))
    p = b.state[0:3, :n].t()[mask]
    want = (torch.tensor([1.0, 2.0, 9.0], device=DEV) - p).norm(dim=1) - 0.5
    assert bool(((rows[_lib.TGT_PREV_DIST][mask] - want).abs() <= 1e-5).all()) and bool((rows[_lib.TGT_CZ][mask] == 9.0).all())
    assert bool((b.captures[mask] == 0).all()) and bool((b.target_position[mask] == torch.tensor([1.0, 2.0, 9.0], device=DEV)).all())
