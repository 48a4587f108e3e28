"""Gate courses on the GPU (include/fpv_abi.h "Gate courses"): on every launch path the 14 state rows of a gate handle
are bit for bit those of a twin without a course, and the race - word, reward, done, observation rows - is bit for bit what the
host's fpv_gate_eval makes of the twin's per-step states; the same bits on partitions, shards, either traversal order, with
in-kernel noise, an object list and across a checkpoint; finishing lanes reset themselves; refusals are by name."""
import functools

import numpy as np
import pytest
import torch

import gate_course as gc
from fpyv_amd import _lib, load_params
from fpyv_amd import gates as G
from fpyv_amd.env import DroneBatch, FpvVecEnv, RacerBatch
from fpyv_amd.objects import Gate
from oracle import lane_model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, STEPS, CHUNK = gc.N, gc.STEPS, 20
G10_OBJECTS = [(2, 1.5, -6.0, 3.0, 0.8, 0.0), (1, 3.0, 0.0, 0.0, 1.0, 5.0), (1, -2.0, 2.5, 0.0, 0.6, 1.5), (0, 0.0, 0.0, 0.0, 0.0, 0.0)]
FINISH = _lib.GATE_EVENT_FINISH


def _start(b, init):
    b.state[:, :b.n] = torch.from_numpy(np.ascontiguousarray(init[:, :b.n])).to(DEV)


def _twin_race(init, acts_np, rows, objects=None, rows_from=None, eval_kw=None, **batch_kw):
    """A twin DroneBatch WITHOUT a course, single steps from `init`; fpv_gate_eval fed with its per-step states.  Returns the
    twin's final state and the per-step expectation: words, rewards, dones, obs.  `rows_from` = (step, rows): the course moves then."""
    n, steps = init.shape[1], acts_np.shape[0]
    twin = DroneBatch(load_params(fps=1000), n, device=DEV, **batch_kw)
    _start(twin, init)
    a = torch.from_numpy(acts_np).to(DEV)
    snaps, dones = [twin.state[:, :n].clone()], []
    for t in range(steps):
        twin.step(None if a is None else a[t], object_list=objects or (), return_imu=False)
        snaps.append(twin.state[:, :n].clone())
        dones.append(twin.done.clone())
    torch.cuda.synchronize()
    S = torch.stack(snaps).cpu().numpy()
    D = torch.stack(dones).cpu().numpy()
    word = np.zeros(n, np.uint32)
    W, R, Dn, O = np.empty((steps, n), np.uint32), np.empty((steps, n), np.float32), np.empty((steps, n), bool), np.empty((steps, n, 6), np.float32)
    for t in range(steps):
        r = rows_from[1] if rows_from is not None and t >= rows_from[0] else rows
        word, R[t], Dn[t], O[t] = G.evaluate(r, S[t, 0:3].T, S[t + 1, 0:3].T, S[t + 1, 6:10].T, D[t], word, **(eval_kw or {}))
        W[t] = word
    return dict(state=S[-1], snaps=S, phys_done=D, words=W, reward=R, done=Dn, obs=O)


@functools.lru_cache(maxsize=None)
def _base():
    """the T2 course and starts: the expectation every plain-handle test shares (computed once, read-only)"""
    p, init, snaps, pdone = gc.trajectory()
    rows = G.derive(gc.course())
    e = _twin_race(init[:, :N], gc.acts(), rows)
    # the twin is the host lane model bit for bit, and nothing ends physically on this course
    assert np.array_equal(e["snaps"].view(np.uint32), snaps.view(np.uint32)) and not e["phys_done"].any()
    return p, np.ascontiguousarray(init[:, :N]), rows, e


def _gate_batch(n=N, **kw):
    return DroneBatch(load_params(fps=1000), n, device=DEV, gates=gc.course(), **kw)


def _same_bits(got, want, what):
    g = np.ascontiguousarray(got.cpu().numpy() if torch.is_tensor(got) else got)
    w = np.ascontiguousarray(want)
    assert g.shape == w.shape and g.dtype.itemsize == w.dtype.itemsize, (what, g.shape, w.shape, g.dtype, w.dtype)
    bad = np.flatnonzero(g.reshape(-1).view(np.uint8) != w.reshape(-1).view(np.uint8))
    assert bad.size == 0, f"{what}: {bad.size} bytes differ, first at element {bad[:4] // g.dtype.itemsize}"


def _check_now(b, e, t, what, outputs=True):
    """the batch after step t (0-based) against the expectation: state, word, reward, done, obs (outputs=False: reward and done
    went to the caller's per-step rows)"""
    n = b.n
    _same_bits(b.state[:, :n], e["snaps"][t + 1], f"{what}: state after step {t}")
    _same_bits(b.gate_word.cpu().numpy().view(np.uint32), e["words"][t], f"{what}: word after step {t}")
    if outputs:
        _same_bits(b.reward, e["reward"][t], f"{what}: reward of step {t}")
        assert np.array_equal(b.done.cpu().numpy(), e["done"][t]), f"{what}: done of step {t}"
    _same_bits(b.gate_obs.contiguous(), e["obs"][t], f"{what}: obs after step {t}")


# ---- G1 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["step", "rollout", "step_n", "graph"])
def test_every_launch_path_is_the_twin_plus_gate_eval(how):
    p, init, rows, e = _base()
    gc.assert_event_floors(e["words"])
    a = torch.from_numpy(gc.acts()).to(DEV)
    b = _gate_batch()
    _start(b, init)
    assert b.algorithmic_bytes() == 133 + 8 + 24
    if how == "step":
        words = np.empty((STEPS, N), np.uint32)
        for t in range(STEPS):
            b.step(a[t], return_imu=False)
            if t % 7 == 0 or t == STEPS - 1:
                _check_now(b, e, t, how)
            words[t] = b.gate_word.cpu().numpy().view(np.uint32)
        _same_bits(words, e["words"], "step: every word")
        assert gc.assert_event_floors(words) == gc.assert_event_floors(e["words"])
        assert torch.equal(b.gate_index, torch.from_numpy((words[-1] & 0xFF).astype(np.int32)).to(DEV))
        assert torch.equal(b.gates_passed, torch.from_numpy((words[-1] >> 10).astype(np.int32)).to(DEV))
        return
    rew, don = torch.zeros((CHUNK, N), device=DEV), torch.zeros((CHUNK, N), dtype=torch.bool, device=DEV)
    kw = dict(rollout=dict(fused=False), step_n=dict(), graph=dict(graph=True))[how]
    for t0 in range(0, STEPS, CHUNK):
        b.rollout(a[t0:t0 + CHUNK], rewards=rew, dones=don, **kw)
        _same_bits(rew, e["reward"][t0:t0 + CHUNK], f"{how}: per-step rewards from step {t0}")
        assert np.array_equal(don.cpu().numpy(), e["done"][t0:t0 + CHUNK]), f"{how}: per-step dones from step {t0}"
        t = t0 + CHUNK - 1
        _same_bits(b.state[:, :N], e["snaps"][t + 1], f"{how}: state after step {t}")
        w = b.gate_word.cpu().numpy().view(np.uint32)
        _same_bits(w, e["words"][t], f"{how}: word after step {t}")
        _same_bits(b.gate_obs.contiguous(), e["obs"][t], f"{how}: obs after step {t}")
    w = b.gate_word.cpu().numpy().view(np.uint32)
    assert ((w >> 10) > 0).sum() >= 100 and (((w >> 10) >= 4) & ((w & 0xFF) == (w >> 10) % 4)).sum() >= 3       # the floors, on the GPU's words


# ---- G2 ---------------------------------------------------------------------------------------------------------------------
def test_quiet_k_step_launch_ends_where_the_single_steps_end():
    p, init, rows, e = _base()
    b = _gate_batch()
    _start(b, init)
    b.rollout(torch.from_numpy(gc.acts()).to(DEV))              # one launch, k = 300, no per-step outputs
    _check_now(b, e, STEPS - 1, "quiet fpv_step_n")
    c = _gate_batch(gate_obs=False)                             # without the observation rows: 141 B, the same race
    _start(c, init)
    c.rollout(torch.from_numpy(gc.acts()).to(DEV))
    assert c.algorithmic_bytes() == 141 and c.gate_obs is None
    assert torch.equal(c.gate_word, b.gate_word) and torch.equal(c.state, b.state) and torch.equal(c.reward, b.reward)


# ---- G3 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_drone", [True, False])
def test_finishing_lanes_reset_themselves(per_drone):
    pos, vel, ypr = gc.starts()
    start = (np.arange(N) % 5 == 0).astype(np.uint8)            # every fifth lane starts (and restarts) at gate 1
    course = gc.course()[:3]
    rows = G.derive(course)
    a = torch.from_numpy(gc.acts()).to(DEV)
    kw = dict(gates=course, laps=1, auto_reset=True, per_drone_reset_pose=per_drone, gate_start=start)

    def fresh():
        b = DroneBatch(load_params(fps=1000), N, device=DEV, **kw)
        if per_drone:
            b.reset(position=pos, velocity=vel, ypr=ypr)
        else:
            b.reset()
            _start(b, gc.trajectory()[1])
        assert torch.equal(b.gate_index, torch.from_numpy(start.astype(np.int32)).to(DEV)) and int(b.gates_passed.sum()) == 0
        return b

    b = fresh()
    finished = np.zeros(N, bool)
    per_step = []
    for t in range(STEPS):
        b.step(a[t], return_imu=False)
        w = b.gate_word.cpu().numpy().view(np.uint32)
        per_step.append((b.reward.clone(), b.done.clone()))
        fin = ((w >> 8) & 3) == FINISH
        if fin.any():
            done = b.done.cpu().numpy()
            assert done[fin].all(), "FINISH must end the episode in that step"
            assert ((w[fin] >> 10) == 0).all() and np.array_equal(w[fin] & 0xFF, start[fin]), "a finished lane restarts at its start gate with nothing passed"
            st = b.state[:, :N].cpu().numpy()
            if per_drone:
                assert np.array_equal(st[0:10, fin], b.reset_pose[:, :N].cpu().numpy()[:, fin]), "... at its own start pose"
            else:
                assert np.allclose(st[0:3, fin].T, load_params(fps=1000).init_position)
            want, scale = gc.obs64(rows, w[fin], st[6:10, fin].T, st[0:3, fin].T)
            got = b.gate_obs.cpu().numpy()[fin]
            assert (np.abs(got - want)[:, :3] <= 16 * gc.EPS32 * scale[:, None]).all() and (np.abs(got - want)[:, 3:] <= 16 * gc.EPS32).all(), \
                "the observation points at the new next gate from the new pose"
            finished |= fin
    assert finished.sum() >= 1, "at least one lane must finish"
    assert finished[start == 0].any()
    # the k-step path: the same bits, per step and at the end
    c = fresh()
    rew, don = torch.zeros((STEPS, N), device=DEV), torch.zeros((STEPS, N), dtype=torch.bool, device=DEV)
    c.rollout(a, rewards=rew, dones=don)
    assert torch.equal(rew, torch.stack([r for r, _ in per_step])) and torch.equal(don, torch.stack([d for _, d in per_step]))
    for name in ("state", "gate_word", "gate_obs_rows"):          # (reward and done went to the per-step rows above)
        assert torch.equal(getattr(c, name), getattr(b, name)), name
    assert int((don & (rew > 40)).sum()) >= finished.sum()          # the finish bonus arrives with the done flag
    # a masked fpv_reset resets only the masked words
    before = b.gate_word.cpu().numpy().view(np.uint32).copy()
    mask = np.arange(N) % 3 == 0
    b.reset(mask=torch.from_numpy(mask).to(DEV))
    after = b.gate_word.cpu().numpy().view(np.uint32)
    assert np.array_equal(after[~mask], before[~mask])
    assert ((after[mask] >> 10) == 0).all() and np.array_equal(after[mask] & 0xFF, start[mask]) and np.array_equal(after[mask] & 0x300, before[mask] & 0x300)
    assert (before[mask] >> 10).sum() > 0, "the reset must have had something to clear"


# ---- G4 ---------------------------------------------------------------------------------------------------------------------
def test_partitions_shards_and_rotation_give_the_same_bits():
    p, init, rows, e = _base()
    a = torch.from_numpy(gc.acts()).to(DEV)
    t_end = 119
    env = FpvVecEnv(p, N, device=DEV, partitions=2, auto_reset=False, track_episodes=False, gates=gc.course())
    assert env.partitions == 2
    _start(env.batch, init)
    torch.cuda.synchronize()
    for t in range(t_end + 1):
        _, _, _, info = env.step(a[t])
    torch.cuda.synchronize()
    _check_now(env.batch, e, t_end, "partitions=2")
    assert np.array_equal(info["gates_passed"].cpu().numpy(), (e["words"][t_end] >> 10).astype(np.int32))
    assert np.array_equal(info["gate_event"].cpu().numpy(), ((e["words"][t_end] >> 8) & 3).astype(np.int32))
    env.close()
    for lo, hi in ((0, 500), (500, N)):                         # two shards: columns of the same population
        s = _gate_batch(hi - lo, drone_id_offset=lo)
        _start(s, init[:, lo:hi])
        for t in range(t_end + 1):
            s.step(a[t, lo:hi].contiguous(), return_imu=False)
        sub = dict(snaps=e["snaps"][:, :, lo:hi], words=e["words"][:, lo:hi], reward=e["reward"][:, lo:hi], done=e["done"][:, lo:hi],
                   obs=e["obs"][:, lo:hi])
        _check_now(s, sub, t_end, f"shard {lo}:{hi}")
    r = _gate_batch()
    r.set_rotation(256)
    assert r.rotation == 256
    _start(r, init)
    for t in range(t_end + 1):
        r.step(a[t], return_imu=False)
    _check_now(r, e, t_end, "set_rotation(256)")


def test_stick_noise_and_a_checkpoint_in_mid_course():
    p, init, rows, _ = _base()
    steps = 120
    acts = gc.acts()[:steps]
    e = _twin_race(init, acts, rows, stick_noise=True, noise_seed=11)
    assert ((e["words"][-1] >> 10) > 0).sum() >= 20
    b = _gate_batch(stick_noise=True, noise_seed=11)
    _start(b, init)
    a = torch.from_numpy(acts).to(DEV)
    for t in range(60):
        b.step(a[t], return_imu=False)
    _check_now(b, e, 59, "stick noise, single steps")
    sd = b.state_dict()
    assert "gate_word" in sd and sd["gate_course"]["count"] == 4
    c = _gate_batch(stick_noise=True, noise_seed=11, gate_rewards=dict(passed=1.0))       # other constants: the checkpoint's win
    c.load_state_dict(sd)
    c.rollout(a[60:])                                           # ... and on through the k-step kernel
    _check_now(c, e, steps - 1, "stick noise, checkpoint, fpv_step_n")


def test_object_list_crash_ends_the_episode_with_the_crash_penalty():
    # the T2 starts and course moved next to the G10 list's cylinder (centre (3, 0), radius 1, 5 m high): gate 0 stands half a
    # metre in front of its wall, so lanes pass it and then fly into the cylinder
    off = np.array([1.0, 0.0, -8.0])
    pos, vel, ypr = gc.starts()
    p = load_params(fps=1000)
    init = lane_model.initial_state(p, N, pos + off, vel, ypr)[:, :N]
    steps = 150
    acts = gc.acts()[:steps]
    course = gc.course()
    for g in course:
        g.position = g.position + off
    rows = G.derive(course)
    rewards = dict(progress=1.0, passed=10.0, finish=50.0, missed=5.0, crash=100.0)
    e = _twin_race(init, acts, rows, objects=G10_OBJECTS, eval_kw=dict(gate_rewards=rewards))
    assert e["phys_done"].sum() >= 100 and (e["reward"][e["phys_done"]] < -50).all(), "a crash must cost the crash penalty"
    assert np.array_equal(e["done"], e["phys_done"]) and ((e["words"][-1] >> 10) > 0).sum() >= 20
    a = torch.from_numpy(acts).to(DEV)
    b = DroneBatch(p, N, device=DEV, gates=course, gate_rewards=rewards)
    _start(b, init)
    for t in range(steps):
        b.step(a[t], object_list=G10_OBJECTS, return_imu=False)
    _check_now(b, e, steps - 1, "object list, single steps")
    c = DroneBatch(p, N, device=DEV, gates=course, gate_rewards=rewards)
    _start(c, init)
    rew, don = torch.zeros((steps, N), device=DEV), torch.zeros((steps, N), dtype=torch.bool, device=DEV)
    c.rollout(a, rewards=rew, dones=don, object_list=G10_OBJECTS)
    _check_now(c, e, steps - 1, "object list, fpv_step_n", outputs=False)
    _same_bits(rew, e["reward"], "object list: per-step rewards")
    assert np.array_equal(don.cpu().numpy(), e["done"])


# ---- G5 ---------------------------------------------------------------------------------------------------------------------
def test_refusals_are_by_name():
    p = load_params(fps=1000)
    a = torch.zeros((64, 4), device=DEV)
    with pytest.raises(_lib.FpvError, match="fp16 state"):
        DroneBatch(p, 64, device=DEV, fp16_state=True, gates=gc.course())
    with pytest.raises(_lib.FpvError, match="Racer mode"):
        RacerBatch(None, 64, device=DEV, gates=gc.course())
    with pytest.raises(_lib.FpvError, match="physics table"):
        DroneBatch(p, 64, device=DEV, per_drone_physics=True, gates=gc.course())
    b = DroneBatch(p, 64, device=DEV, kahan_position=True, gates=gc.course())
    with pytest.raises(_lib.FpvError, match="Kahan rows"):
        b.step(a, return_imu=False)
    b = DroneBatch(p, 64, device=DEV, with_obs_aos=True, gates=gc.course())
    with pytest.raises(_lib.FpvError, match="AoS head"):
        b.step(a, return_imu=False)
    b = _gate_batch(64)
    with pytest.raises(_lib.FpvError, match="guidance override"):
        b.step(a, rotation_matrix=np.eye(3), thrust_force=1.0, return_imu=False)
    b.step(a, return_imu=False)                                 # ... and the refused call left nothing behind
    with pytest.raises(_lib.FpvError, match="gate course"):
        _lib.check(b._L.fpv_set_physics(b._handle, b.state.data_ptr(), b.ld))
    n = DroneBatch(p, 64, device=DEV, stick_noise=True, gates=gc.course())
    with pytest.raises(_lib.FpvError, match="stick noise AND an object list"):
        n.step(a, object_list=G10_OBJECTS, return_imu=False)
    with pytest.raises(ValueError, match="without gates="):
        DroneBatch(p, 64, device=DEV).set_gates(gc.course())


def test_unbinding_and_moving_gates():
    p, init, rows, e = _base()
    a = torch.from_numpy(gc.acts()).to(DEV)
    b = _gate_batch()
    _start(b, init)
    for t in range(40):
        b.step(a[t], return_imu=False)
    _check_now(b, e, 39, "before unbinding")
    b.set_gates(None)                                           # the plain kernels again: 133 B, the goal reward, the twin's state
    assert b.algorithmic_bytes() == 133
    word = b.gate_word.clone()
    twin = DroneBatch(p, N, device=DEV)
    _start(twin, e["snaps"][40])
    for t in range(40, 80):
        b.step(a[t], return_imu=False)
        twin.step(a[t], return_imu=False)
    assert torch.equal(b.state, twin.state) and torch.equal(b.reward, twin.reward) and torch.equal(b.gate_word, word)
    _same_bits(b.state[:, :N], e["snaps"][80], "unbound: state")
    # moving gates: set_gates between steps takes effect at the next step
    moved = gc.course()
    for g, dx in zip(moved, (0.25, -0.1, 0.2, 0.15)):
        g.position = g.position + np.array([dx, 0.05, -0.05])
    m = _twin_race(init, gc.acts()[:120], rows, rows_from=(30, G.derive(moved)))
    assert not np.array_equal(m["words"][-1], e["words"][119]), "the moved course must change the race"
    c = _gate_batch()
    _start(c, init)
    for t in range(30):
        c.step(a[t], return_imu=False)
    c.set_gates(moved)
    for t in range(30, 75):
        c.step(a[t], return_imu=False)
    _check_now(c, m, 74, "moved gates, single steps")
    c.rollout(a[75:120])
    _check_now(c, m, 119, "moved gates, fpv_step_n")


# ---- every course row on every multi-step call -------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["rollout", "step_n", "graph"])
@pytest.mark.parametrize("row", ["plain", "objects", "noise", "reset_pose"])
def test_course_rows_on_the_multi_step_calls_equal_single_steps(row, how):
    """A course alone, with an object list, with stick noise and with a reset-pose table under a ceiling that resets lanes at
    once: fpv_rollout, fpv_step_n and fpv_rollout_graph (with an object list, stick noise or a reset source handed on to
    fpv_step_n) leave the bits of the same handle type stepped with fpv_step - 1000 drones, two calls of k = 5."""
    k = 5
    p = load_params(fps=1000, ceiling=10.2) if row == "reset_pose" else load_params(fps=1000)
    kw = dict(objects={}, plain={}, noise=dict(stick_noise=True, noise_seed=11), reset_pose=dict(auto_reset=True, per_drone_reset_pose=True))[row]
    objects = G10_OBJECTS if row == "objects" else None
    pos, vel, ypr = gc.starts()
    a = torch.from_numpy(gc.acts()[:2 * k]).to(DEV)
    one, many = (DroneBatch(p, N, device=DEV, gates=gc.course(), **kw) for _ in range(2))
    for b in (one, many):
        b.reset(position=pos, velocity=vel, ypr=ypr)
    resets = 0
    for t in range(2 * k):
        one.step(a[t], object_list=objects or (), return_imu=False)
        resets += int(one.done.sum())
    for c in range(2):
        many.rollout(a[c * k:(c + 1) * k], object_list=objects, **dict(rollout=dict(fused=False), step_n={}, graph=dict(graph=True))[how])
    assert one.step_counter() == many.step_counter() == 2 * k
    for name in ("state", "gate_word", "gate_obs_rows", "reward", "done", "noise_state"):
        x, y = getattr(one, name), getattr(many, name)
        assert (x is None and y is None) or torch.equal(x.view(torch.uint8), y.view(torch.uint8)), name
    assert row != "reset_pose" or resets > N, "the ceiling must reset lanes in these steps"
