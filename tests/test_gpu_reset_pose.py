"""Reset sources on the GPU (include/fpv_abi.h "Reset sources", ABI 9): the per-drone reset-pose table survives the in-kernel
auto-reset, the jitter is exactly fpv_reset_pose_sample's arithmetic, and every path - fpv_step, fpv_rollout, fpv_step_n,
fpv_rollout_graph, partitions, shards, fp16 state, the AoS head, object lists, checkpoints - gives the same bits."""
import ctypes as C

import numpy as np
import pytest
import torch

from fpyv_amd import _lib, load_params
from fpyv_amd.env import DroneBatch, FpvVecEnv
from oracle import oracle
from parity import assert_parity, soa_vs_oracle

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CEIL = 10.2
JIT = dict(reset_position_range=[[-0.5, -0.5, -0.05], [0.5, 0.5, 0.05]], reset_velocity_range=[[-0.2, -0.2, 0.0], [0.2, 0.2, 0.5]],
           reset_ypr_range_deg=[[-15.0, -15.0, -180.0], [15.0, 15.0, 180.0]], reset_seed=0xC0FFEE_1234)


def _params(jitter=False):
    return load_params(fps=1000, ceiling=CEIL, **(JIT if jitter else {}))


def _starts(n, seed=0):
    """per-drone starts just below the ceiling, climbing: most lanes end an episode every few dozen steps"""
    rng = np.random.default_rng(seed)
    pos = np.stack([rng.uniform(-5, 5, n), rng.uniform(-5, 5, n), rng.uniform(10.0, 10.1, n)], 1).astype(np.float32)
    vel = np.stack([rng.uniform(-1, 1, n), rng.uniform(-1, 1, n), rng.uniform(1.5, 4.0, n)], 1).astype(np.float32)
    ypr = rng.uniform(-20, 20, (n, 3)).astype(np.float32)
    return pos, vel, ypr


def _batch(n, jitter=False, table=True, seed=0, **kw):
    kw.setdefault("auto_reset", True)
    b = DroneBatch(_params(jitter), n, device=DEV, per_drone_reset_pose=table, **kw)
    pos, vel, ypr = _starts(n, seed)
    b.reset(position=pos, velocity=vel, ypr=ypr)
    return b


def _actions(steps, n, seed=1):
    g = torch.Generator(device=DEV).manual_seed(seed)
    a = torch.rand((steps, n, 4), generator=g, device=DEV) * 2 - 1
    a[..., 3] = a[..., 3] * 0.3 + 0.1
    return a


def _sample(cp, gid, step, e, base):
    b = np.ascontiguousarray(base, dtype=np.float32)
    out = np.empty(10, dtype=np.float32)
    assert _lib.lib().fpv_reset_pose_sample(C.byref(cp), int(gid), int(step), int(e), b.ctypes.data, out.ctypes.data) == 0
    return out


def _bits(t):
    return t.contiguous().view(torch.int32).cpu()


@pytest.mark.parametrize("n", [4096, 1000])
def test_auto_reset_returns_every_drone_to_its_own_start(n):
    b = _batch(n)
    start = b.state[:10, :n].clone()
    assert torch.equal(b.reset_pose[:, :n], start)
    acts, resets = _actions(200, n), 0
    for t in range(200):
        b.step(acts[t], return_imu=False)
        d = b.done.clone()
        if d.any():
            resets += int(d.sum())
            assert torch.equal(_bits(b.state[:10, :n][:, d]), _bits(start[:, d])), t
            assert torch.all(b.state[10:14, :n][:, d] == 0)
    assert resets > 2 * n, resets                                    # several episodes per lane
    assert torch.equal(b.reset_pose[:, :n], start)                  # the in-kernel reset only reads the table


def test_jitter_is_the_host_sample_and_stays_in_its_box():
    n = 2048
    b = _batch(n, jitter=True)
    cp = b._cparams
    base = b.reset_pose[:, :n].cpu().numpy()
    st = b.state[:10, :n].cpu().numpy()
    for i in range(0, n, 97):                                       # explicit reset: e = 1, t = the counter at the call (0)
        assert _sample(cp, i, 0, 1, base[:, i]).view(np.uint32).tolist() == st[:, i].view(np.uint32).tolist()
    lo = np.array(JIT["reset_position_range"][0] + JIT["reset_velocity_range"][0], dtype=np.float64)
    hi = np.array(JIT["reset_position_range"][1] + JIT["reset_velocity_range"][1], dtype=np.float64)
    acts, checked = _actions(200, n, seed=3), 0
    for t in range(200):
        b.step(acts[t], return_imu=False)
        d = torch.nonzero(b.done).flatten().cpu().numpy()
        if len(d):
            st = b.state[:10, :n].cpu().numpy()
            for i in d[:16]:
                want = _sample(cp, i, t, 0, base[:, i])
                assert want.view(np.uint32).tolist() == st[:, i].view(np.uint32).tolist(), (t, i)
                off = st[:6, i].astype(np.float64) - base[:6, i]
                assert np.all(off >= lo - 1e-5) and np.all(off <= hi + 1e-5)
                checked += 1
    assert checked > 200
    b.reset(mask=torch.arange(n, device=DEV) % 3 == 0)              # explicit reset later in the run: e = 1 at t = 200
    st = b.state[:10, :n].cpu().numpy()
    for i in range(0, n, 3 * 31):
        assert _sample(cp, i, 200, 1, base[:, i]).view(np.uint32).tolist() == st[:, i].view(np.uint32).tolist()


def _full(b):
    n = b.n
    return [b.state[:, :n], b.noise_state[:, :n], b.reset_pose[:, :n], b.ep_return, b.ep_length, b.last_return, b.last_length,
            b.reward, b.done]


def _same(x, y):
    for u, v in zip(_full(x), _full(y)):
        assert torch.equal(u.contiguous().view(torch.uint8), v.contiguous().view(torch.uint8))


def test_every_path_gives_the_same_bits():
    n, k, chunks = 3000, 30, 10
    kw = dict(jitter=True, stick_noise=True, noise_seed=99, track_episodes=True)
    ref = _batch(n, **kw)
    for t in range(k * chunks):
        ref.step(None, return_imu=False)
    for how in ("rollout", "step_n", "graph"):
        b = _batch(n, **kw)
        for c in range(chunks):
            if how == "rollout":
                b.rollout(None, steps=k, fused=False)              # fpv_rollout: k issued single-step launches
            elif how == "step_n":
                b.rollout(None, steps=k)                           # fpv_step_n: one launch
            else:
                b.rollout(None, steps=k, graph=True)               # fpv_rollout_graph
        _same(ref, b)
        assert int(ref.last_length.max()) > 0
    # table only (no jitter, caller sticks): the graph may replay - same bits as the issued steps
    acts = _actions(k * chunks, n, seed=5)
    r2, g2 = _batch(n, track_episodes=True), _batch(n, track_episodes=True)
    for t in range(k * chunks):
        r2.step(acts[t], return_imu=False)
    for c in range(chunks):
        g2.rollout(acts[c * k:(c + 1) * k].contiguous(), graph=True)
    assert torch.equal(r2.state, g2.state) and torch.equal(r2.ep_return, g2.ep_return) and torch.equal(r2.last_length, g2.last_length)


def test_partitions_and_shards_match_the_single_batch():
    n, steps = 4096, 300
    pos, vel, ypr = _starts(n, 7)
    opts = dict(per_drone_reset_pose=True, stick_noise=True, noise_seed=5, track_episodes=True)
    envs = [FpvVecEnv(_params(True), n, device=DEV, partitions=p, **opts) for p in (1, 2)]
    assert envs[1].partitions == 2
    for e in envs:
        e.reset(position=pos, velocity=vel, ypr=ypr)
    for t in range(steps):
        for e in envs:
            e.step(None)
        if t == 150:
            for e in envs:
                e.reset(mask=torch.arange(n, device=DEV) % 5 == 0)  # explicit jittered reset mid-run
    torch.cuda.synchronize()
    _same(envs[0].batch, envs[1].batch)
    # two handles over column ranges (dist.py's shards): global ids through drone_id_offset
    h = n // 2
    shards = []
    for lo in (0, h):
        s = DroneBatch(_params(True), h, device=DEV, auto_reset=True, drone_id_offset=lo, **opts)
        s.reset(position=pos[lo:lo + h], velocity=vel[lo:lo + h], ypr=ypr[lo:lo + h])
        shards.append(s)
    one = DroneBatch(_params(True), n, device=DEV, auto_reset=True, **opts)
    one.reset(position=pos, velocity=vel, ypr=ypr)
    for t in range(steps):
        one.step(None, return_imu=False)
        for s in shards:
            s.step(None, return_imu=False)
    for k, s in enumerate(shards):
        assert torch.equal(s.state[:, :h], one.state[:, k * h:(k + 1) * h])
        assert torch.equal(s.reset_pose[:, :h], one.reset_pose[:, k * h:(k + 1) * h])
    for e in envs:
        e.close()


def test_oracle_replays_each_episode_from_the_pose_it_was_given():
    n, steps = 2048, 200
    b = _batch(n, jitter=True)
    p = b.params
    idx = np.random.default_rng(4).choice(n, 64, replace=False)
    acts = _actions(steps, n, seed=9)
    hist, dones = np.empty((steps, 14, 64), np.float32), np.empty((steps, 64), bool)
    for t in range(steps):
        b.step(acts[t], return_imu=False)
        hist[t] = b.state[:, idx].cpu().numpy()
        dones[t] = b.done[idx].cpu().numpy()
    a_host = acts[:, idx].cpu().numpy().astype(np.float64)
    replayed = 0
    for j in range(64):
        ends = np.flatnonzero(dones[:, j])
        if len(ends) < 2 or ends[1] - ends[0] < 3:
            continue
        t0, t1 = ends[0], ends[1] - 1                   # the episode that began with the reset at step t0
        s0 = hist[t0, :, j].astype(np.float64)
        ref = np.zeros((1, oracle.DRONE_STATE))
        ref[0, 0:6] = s0[0:6]
        ref[0, 6:15] = oracle.quat_to_matrix(s0[6:10][None])[0].reshape(9)
        oracle.drone_run(p, ref, np.ascontiguousarray(a_host[t0 + 1:t1 + 1, j:j + 1]))
        assert_parity(soa_vs_oracle(hist[t1, :, j:j + 1], ref, 1), 1e-5, f"drone {idx[j]}")
        replayed += 1
    assert replayed >= 32


def test_fp16_state_resets_to_the_encoded_pose_and_kstep_matches():
    n, steps = 2048, 200
    a, b = _batch(n, jitter=True, fp16_state=True), _batch(n, jitter=True, fp16_state=True)
    base = a.reset_pose[:, :n].cpu().numpy()
    acts, checked = _actions(steps, n, seed=11), 0
    for t in range(steps):
        a.step(acts[t], return_imu=False)
        d = torch.nonzero(a.done).flatten().cpu().numpy()
        if len(d):
            w = a.rows_f32(0, 10).cpu().numpy()
            for i in d[:8]:
                want = _sample(a._cparams, i, t, 0, base[:, i])
                assert np.array_equal(w[i, :3], want[:3])                                   # position rows stay fp32
                assert np.allclose(w[i, 3:6], want[3:6], rtol=1e-4, atol=1e-4)              # v: binary16 + 5 low bits
                sgn = 1.0 if np.dot(w[i, 6:10], want[6:10]) >= 0 else -1.0                 # q and -q: the same attitude; the
                assert np.abs(sgn * w[i, 6:10] - want[6:10]).max() < 1e-4                   # encoding keeps the largest component > 0
                checked += 1
    assert checked > 50
    b.rollout(acts)                                                                         # the k-step kernel: one launch
    assert torch.equal(a.state, b.state) and torch.equal(a.state_h.view(torch.int16), b.state_h.view(torch.int16))


@pytest.mark.parametrize("how", ["aos", "objects"])
def test_aos_head_and_object_list_keep_the_starts(how):
    from fpyv_amd.objects import Ground
    n = 2048
    kw = dict(with_obs_aos=True) if how == "aos" else {}
    b, ref = _batch(n, **kw), _batch(n)
    start = b.state[:10, :n].clone()
    acts, resets = _actions(200, n, seed=13), 0
    for t in range(200):
        if how == "aos":
            b.step(acts[t], return_imu=False)
            ref.step(acts[t], return_imu=False)
            assert torch.equal(b.obs_aos[:, :13], b.state[:13, :n].t())
        else:
            b.step(acts[t], object_list=[Ground()], return_imu=False)
        d = b.done.clone()
        resets += int(d.sum())
        if d.any():
            assert torch.equal(_bits(b.state[:10, :n][:, d]), _bits(start[:, d]))
    assert resets > n
    if how == "aos":
        assert torch.equal(b.state, ref.state)                     # the AoS kernel's branch = the routed k-step kernel's


def test_checkpoint_continues_bit_for_bit():
    n = 2048
    kw = dict(jitter=True, stick_noise=True, noise_seed=3, track_episodes=True)
    a = _batch(n, **kw)
    for t in range(120):
        a.step(None, return_imu=False)
    ck = a.state_dict()
    assert "reset_pose" in ck
    b = DroneBatch(_params(True), n, device=DEV, auto_reset=True, per_drone_reset_pose=True, stick_noise=True, noise_seed=3,
                   track_episodes=True)
    b.load_state_dict(ck)
    for t in range(150):
        a.step(None, return_imu=False)
        b.step(None, return_imu=False)
    _same(a, b)


def test_guidance_override_and_racer_refuse_a_reset_source():
    b = _batch(256)
    with pytest.raises(_lib.FpvError) as e:
        b.step(np.zeros(4, np.float32), rotation_matrix=np.eye(3, dtype=np.float32), thrust_force=5.0, return_imu=False)
    assert e.value.code == -1
    from fpyv_amd.env import RacerBatch
    with pytest.raises(ValueError):
        RacerBatch(None, 256, device=DEV, per_drone_reset_pose=True)


@pytest.mark.parametrize("row,how", [(r, h) for r in ("table", "jitter", "aos", "fp16") for h in ("rollout", "step_n", "graph")
                                     if (r, h) != ("aos", "step_n")])          # (fpv_step_n writes no AoS head)
def test_reset_source_rows_on_the_multi_step_calls_equal_single_steps(row, how):
    """The reset-pose table, the jitter, the table with the AoS head and with fp16 state: fpv_rollout, fpv_step_n and
    fpv_rollout_graph (which hands a reset source on to fpv_step_n, or to fpv_rollout when the AoS head is written) leave the
    bits of the same handle type stepped with fpv_step - 1000 drones, two calls of k = 5, many lanes above the ceiling at once."""
    n, k = 1000, 5
    kw = dict(table={}, jitter=dict(jitter=True), aos=dict(with_obs_aos=True), fp16=dict(fp16_state=True, rounding_seed=7))[row]
    one, many = _batch(n, **kw), _batch(n, **kw)
    for b in (one, many):
        b.state[2] += 0.15                                          # the position rows are fp32 in either layout
    acts, resets = _actions(2 * k, n, seed=17), 0
    for t in range(2 * k):
        one.step(acts[t], return_imu=False)
        resets += int(one.done.sum())
    for c in range(2):
        many.rollout(acts[c * k:(c + 1) * k], **dict(rollout=dict(fused=False), step_n={}, graph=dict(graph=True))[how])
    assert resets > n // 4 and one.step_counter() == many.step_counter() == 2 * k
    for name in ("state", "state_h", "obs_aos", "reward", "done"):
        x, y = getattr(one, name), getattr(many, name)
        assert (x is None and y is None) or torch.equal(x.view(torch.uint8), y.view(torch.uint8)), name
