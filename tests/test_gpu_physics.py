"""Per-drone physics on the GPU (include/fpv_abi.h "Per-drone physics"): every drone of a table handle steps bit for
bit like the host lane model run with ITS parameter set - through fpv_step, fpv_rollout, fpv_step_n and fpv_rollout_graph, with
the ground flag, an object list and in-kernel noise -, holds the oracle's 1e-5, and gives the same bits on partitions, shards,
either traversal order, with reset sources and across a checkpoint."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from fpyv_amd import _lib, load_params
from fpyv_amd.env import DroneBatch, FpvVecEnv, RacerBatch
from oracle import lane_model, oracle
from parity import assert_parity, soa_vs_oracle
from physics_sets import dealt, parameter_sets

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G10_OBJECTS = [(2, 1.5, -6.0, 3.0, 0.8, 0.0), (1, 3.0, 0.0, 0.0, 1.0, 5.0), (1, -2.0, 2.5, 0.0, 0.6, 1.5), (0, 0.0, 0.0, 0.0, 0.0, 0.0)]
RANGES = dict(mass=(0.7, 1.4), thrust=(0.8, 1.25), drag=(0.5, 2.0), rates_lag=(0.6, 1.1), thrust_lag=(0.9, 1.5))


def _acts(steps, n, seed=21):
    rng = np.random.default_rng(seed)
    a = rng.random((steps, n, 4), dtype=np.float32) * 2 - 1
    a[..., 3] = a[..., 3] * 0.4 + 0.1
    return a


def _deal(b, sets):
    which, inp = dealt(sets, b.n)
    b.set_physics(mass=inp[:, 0], thrust_poly=inp[:, 1:5], drag_coefficients=inp[:, 5:8], rates_transition_rate=inp[:, 8],
                  thrust_transition_rate=inp[:, 9])
    return which


def _table_batch(base, n, sets, **kw):
    b = DroneBatch(base, n, device=DEV, per_drone_physics=True, **kw)
    return b, _deal(b, sets)


def _poses(case, n):
    """per-drone starts that exercise the case: near the ground plane for the ground flag, the G10 capture's starts (tiled) for
    its object list"""
    rng = np.random.default_rng(8)
    if case == "ground":
        pos = np.stack([rng.uniform(-3, 3, n), rng.uniform(-3, 3, n), rng.uniform(0.03, 0.14, n)], 1)
        vel = np.stack([rng.uniform(-1, 1, n), rng.uniform(-1, 1, n), rng.uniform(-1.5, 0.0, n)], 1)
        return pos, vel, rng.uniform(-8, 8, (n, 3))
    if case == "objects":
        g = load_golden("g10_objects")
        k = np.arange(n) % g["init_position"].shape[0]
        return g["init_position"][k], g["init_velocity"][k], g["init_ypr"][k]
    return None, None, None


def _expected(sets, which, init, acts, objects=()):
    """the host lane model, one run per parameter set on that set's columns"""
    out = np.empty((14, len(which)), np.float32)
    try:
        lane_model.set_objects(objects)
        for k, p in enumerate(sets):
            idx = np.flatnonzero(which == k)
            m = np.ascontiguousarray(init[:, idx])
            lane_model.run(p, m, np.ascontiguousarray(acts[:, idx]))
            out[:, idx] = m
    finally:
        lane_model.set_objects(())
    return out


def _run(b, how, a, objects=None):
    k, n = a.shape[0], b.n
    if how == "step":
        for t in range(k):
            b.step(a[t], object_list=objects or (), return_imu=False)
    elif how == "rollout":
        b.rollout(a, fused=False, object_list=objects)                                  # fpv_rollout: k issued launches
    elif how == "step_n":
        rew, don = torch.zeros((k, n), device=DEV), torch.zeros((k, n), dtype=torch.bool, device=DEV)
        b.rollout(a, rewards=rew, dones=don, object_list=objects)                       # fpv_step_n with per-step outputs
        return rew, don
    else:
        b.rollout(a, graph=True, object_list=objects)                                   # fpv_rollout_graph
    return None


@pytest.mark.parametrize("n", [4096, 1000])
@pytest.mark.parametrize("case", ["plain", "ground", "objects"])
def test_every_column_is_the_lane_model_of_its_parameter_set(n, case):
    steps = 300
    base = load_params(fps=1000, **(dict(ground=True, ground_damping=2.0) if case == "ground" else {}))
    sets = parameter_sets(base)
    objects = G10_OBJECTS if case == "objects" else None
    acts = _acts(steps, n)
    a = torch.from_numpy(acts).to(DEV)
    init = lane_model.initial_state(base, n, *_poses(case, n))
    which = dealt(sets, n)[0]
    want = _expected(sets, which, init, acts, objects or ())
    assert len({want[:, i].tobytes() for i in range(8)}) == 8, "the eight airframes must fly apart"
    per_step = None
    for how in ("step", "rollout", "step_n", "graph"):
        b, _ = _table_batch(base, n, sets)
        b.state[:, :n] = torch.from_numpy(init[:, :n]).to(DEV)
        out = _run(b, how, a, objects)
        torch.cuda.synchronize()
        got = b.state[:, :n].cpu().numpy()
        bad = np.flatnonzero((got.view(np.uint32) != want.view(np.uint32)).any(axis=0))
        assert bad.size == 0, f"{how}: {bad.size} columns differ from the lane model of their set, first {bad[:5]} (sets {which[bad[:5]]})"
        assert b.algorithmic_bytes() == (177 if case == "plain" else 185)
        if how == "step_n":
            per_step = out
    # the per-step outputs of fpv_step_n: the last row is what the single steps left
    c, _ = _table_batch(base, n, sets)
    c.state[:, :n] = torch.from_numpy(init[:, :n]).to(DEV)
    _run(c, "step", a, objects)
    assert torch.equal(per_step[0][-1], c.reward) and torch.equal(per_step[1][-1], c.done)
    if case != "plain":
        assert bool(per_step[1].any()), "some drone must touch something in this case"


@pytest.mark.parametrize("n", [4096, 1000])
def test_in_kernel_noise_matches_a_homogeneous_batch_of_each_set(n):
    steps, off = 300, (1 << 33) + 640
    base = load_params(fps=1000)
    sets = parameter_sets(base)
    kw = dict(stick_noise=True, noise_seed=9, drone_id_offset=off)
    one, which = _table_batch(base, n, sets, **kw)
    fused, _ = _table_batch(base, n, sets, **kw)
    one.reset(); fused.reset()
    for t in range(steps):
        one.step(None, return_imu=False)
    fused.rollout(None, steps=steps)
    assert torch.equal(one.state, fused.state) and torch.equal(one.noise_state, fused.noise_state)
    for k, p in enumerate(sets):
        h = DroneBatch(p, n, device=DEV, **kw)
        h.reset()
        h.rollout(None, steps=steps)
        idx = torch.from_numpy(np.flatnonzero(which == k)).to(DEV)
        assert torch.equal(one.state[:, idx].view(torch.int32), h.state[:, idx].view(torch.int32)), k
        assert torch.equal(one.noise_state[:, idx], h.noise_state[:, idx]), k


def test_oracle_parity_of_every_set_after_1000_steps():
    """The sets were chosen on the CPU: the lane model holds 1e-5 against the oracle for each of them with these sticks (worst
    position error 2.2e-6, quaternion 4.0e-7), so the GPU is asked for nothing the arithmetic cannot give."""
    n, steps = 4096, 1000
    base = load_params(fps=1000)
    sets = parameter_sets(base)
    acts = _acts(steps, n, seed=21)
    b, which = _table_batch(base, n, sets)
    b.reset()
    b.rollout(torch.from_numpy(acts).to(DEV))
    torch.cuda.synchronize()
    got = b.state.cpu().numpy()
    for k, p in enumerate(sets):
        idx = np.flatnonzero(which == k)
        ref = oracle.drone_initial_state(len(idx), p.init_position, p.init_velocity, p.init_orientation_deg)
        oracle.drone_run(p, ref, np.ascontiguousarray(acts[:, idx]).astype(np.float64))
        err = soa_vs_oracle(np.ascontiguousarray(got[:, idx]), ref, len(idx))
        print(f"set {k}: " + ", ".join(f"{m} {v:.2e}" for m, v in err.items()))
        assert_parity(err, 1e-5, f"set {k}")


def test_a_table_of_the_base_parameters_changes_nothing():
    n, steps = 3000, 200
    for base in (load_params(fps=1000), load_params(fps=1000, ground=True, init_position=np.array([0.0, 0.0, 0.13]))):
        a = torch.from_numpy(_acts(steps, n, seed=2)).to(DEV)
        plain, table = DroneBatch(base, n, device=DEV), DroneBatch(base, n, device=DEV, per_drone_physics=True)
        assert plain.algorithmic_bytes() == 133 and table.algorithmic_bytes() == (185 if base.ground else 177)
        plain.reset(); table.reset()
        for t in range(steps):
            plain.step(a[t], return_imu=False)
            table.step(a[t], return_imu=False)
        assert torch.equal(plain.state.view(torch.int32), table.state.view(torch.int32))
        assert torch.equal(plain.reward, table.reward) and torch.equal(plain.done, table.done) and torch.equal(plain.accel, table.accel)
        plain.rollout(a); table.rollout(a)
        assert torch.equal(plain.state.view(torch.int32), table.state.view(torch.int32))
        plain.rollout(a, graph=True); table.rollout(a, graph=True)
        assert torch.equal(plain.state.view(torch.int32), table.state.view(torch.int32))


def test_set_physics_with_a_mask_moves_only_the_masked_columns():
    n, steps = 2048, 100
    base = load_params(fps=1000)
    a = torch.from_numpy(_acts(steps, n, seed=4)).to(DEV)
    ref, b = DroneBatch(base, n, device=DEV, per_drone_physics=True), DroneBatch(base, n, device=DEV, per_drone_physics=True)
    mask = torch.arange(n, device=DEV) % 3 == 1
    before = b.physics.clone()
    b.set_physics(mass=1.1, thrust_scale=0.9, drag_coefficients=[1.0, 2.0, 3.0], mask=mask)
    assert torch.equal(b.physics[:, :n][:, ~mask], before[:, :n][:, ~mask]) and not torch.equal(b.physics[:, :n][:, mask], before[:, :n][:, mask])
    ref.reset(); b.reset()
    ref.rollout(a); b.rollout(a)
    same = (ref.state[:, :n].view(torch.int32) == b.state[:, :n].view(torch.int32)).all(dim=0)
    assert bool(same[~mask].all()) and not bool(same[mask].any())
    with pytest.raises(_lib.FpvError, match="drone 5"):
        m = np.full(n, 0.75)
        m[5] = -1.0
        b.set_physics(mass=m)
    with pytest.raises(ValueError, match="per_drone_physics"):
        DroneBatch(base, 64, device=DEV).set_physics(mass=1.0)


def test_partitions_shards_and_both_traversal_orders_give_the_same_bits():
    n, steps, seed = 4096, 200, 0xABCDEF
    base = load_params(fps=1000, ceiling=10.3)
    acts = _acts(steps, n, seed=6)
    a = torch.from_numpy(acts).to(DEV)
    # partitions: step_async / step_wait on two column ranges of the one table
    envs = [FpvVecEnv(base, n, device=DEV, partitions=p, per_drone_physics=True) for p in (1, 2)]
    assert envs[1].partitions == 2
    for e in envs:
        e.randomize_physics(seed, **RANGES)
        e.reset()
    assert torch.equal(envs[0].batch.physics, envs[1].batch.physics)
    for t in range(steps):
        envs[0].step(a[t])
        for k in range(2):
            lo, hi = envs[1].partition_range(k)
            envs[1].step_wait(k)
            envs[1].step_async(k, a[t, lo:hi])
        if t == 100:        # a whole-population call between steps in flight: ordered like reset
            m = torch.arange(n, device=DEV) % 7 == 0
            for e in envs:
                e.set_physics(mass=0.9, mask=m)
    for k in range(2):
        envs[1].step_wait(k)
    torch.cuda.synchronize()
    for name in ("state", "reward", "done", "ep_return", "last_length", "physics"):
        x, y = getattr(envs[0].batch, name), getattr(envs[1].batch, name)
        assert torch.equal(x.view(torch.uint8), y.view(torch.uint8)), name
    assert int(envs[0].batch.last_length.max()) > 0, "auto-reset must have fired under the ceiling"
    # two shards with drone_id_offset: the same table and the same trajectories as the whole
    h = n // 2
    one = DroneBatch(base, n, device=DEV, per_drone_physics=True, drone_id_offset=1 << 40)
    one.randomize_physics(seed, **RANGES)
    one.reset()
    one.set_rotation(0)                                       # the plain order ...
    rot = DroneBatch(base, n, device=DEV, per_drone_physics=True, drone_id_offset=1 << 40)
    rot.randomize_physics(seed, **RANGES)
    rot.reset()
    rot.set_rotation(1024)                                    # ... and a rotated one
    assert rot.rotation == 1024 and one.rotation == 0
    shards = []
    for lo in (0, h):
        s = DroneBatch(base, h, device=DEV, per_drone_physics=True, drone_id_offset=(1 << 40) + lo)
        s.randomize_physics(seed, **RANGES)
        s.reset()
        assert torch.equal(s.physics[:, :h], one.physics[:, lo:lo + h])
        shards.append(s)
    for t in range(steps):
        one.step(a[t], return_imu=False)
        rot.step(a[t], return_imu=False)
        for k, s in enumerate(shards):
            s.step(a[t, k * h:(k + 1) * h], return_imu=False)
    assert torch.equal(one.state.view(torch.int32), rot.state.view(torch.int32))
    for k, s in enumerate(shards):
        assert torch.equal(s.state[:, :h].view(torch.int32), one.state[:, k * h:(k + 1) * h].view(torch.int32))
    assert len(torch.unique(one.physics[10, :n])) > n // 2    # the masses really differ
    for e in envs:
        e.close()


JIT = dict(reset_position_range=[[-0.5, -0.5, -0.05], [0.5, 0.5, 0.05]], reset_velocity_range=[[-0.2, -0.2, 0.0], [0.2, 0.2, 0.5]],
           reset_ypr_range_deg=[[-15.0, -15.0, -180.0], [15.0, 15.0, 180.0]], reset_seed=0xC0FFEE_1234)


def _starts(n, seed=0):
    rng = np.random.default_rng(seed)
    pos = np.stack([rng.uniform(-5, 5, n), rng.uniform(-5, 5, n), rng.uniform(10.0, 10.1, n)], 1).astype(np.float32)
    vel = np.stack([rng.uniform(-1, 1, n), rng.uniform(-1, 1, n), rng.uniform(1.5, 4.0, n)], 1).astype(np.float32)
    return pos, vel, rng.uniform(-20, 20, (n, 3)).astype(np.float32)


def test_reset_sources_combine_with_the_table():
    """Per-drone starts, jitter and auto-reset under a tight ceiling (tests/test_gpu_reset_pose.py) on a table handle: single steps
    (routed to the k-step kernel, k = 1) and fpv_step_n agree bitwise, and a lane that resets keeps its physics - the columns of
    a set equal a homogeneous handle of that set with the same reset sources and global ids."""
    n, steps = 2048, 200
    base = load_params(fps=1000, ceiling=10.2, **JIT)
    sets = parameter_sets(base)
    pos, vel, ypr = _starts(n)
    a = torch.from_numpy(_acts(steps, n, seed=12)).to(DEV)
    kw = dict(auto_reset=True, per_drone_reset_pose=True, track_episodes=True)
    one, which = _table_batch(base, n, sets, **kw)
    fused, _ = _table_batch(base, n, sets, **kw)
    table0 = one.physics.clone()
    for b in (one, fused):
        b.reset(position=pos, velocity=vel, ypr=ypr)
    resets = 0
    for t in range(steps):
        one.step(a[t], return_imu=False)
        resets += int(one.done.sum())
    fused.rollout(a)
    assert resets > 2 * n
    for name in ("state", "ep_return", "ep_length", "last_return", "last_length", "reward", "done"):
        assert torch.equal(getattr(one, name).view(torch.uint8), getattr(fused, name).view(torch.uint8)), name
    assert torch.equal(one.physics, table0)
    for k in (0, 3, 6):
        h = DroneBatch(sets[k], n, device=DEV, **kw)
        h.reset(position=pos, velocity=vel, ypr=ypr)
        h.rollout(a)
        idx = torch.from_numpy(np.flatnonzero(which == k)).to(DEV)
        assert torch.equal(one.state[:, idx].view(torch.int32), h.state[:, idx].view(torch.int32)), k
        assert torch.equal(one.last_length[idx], h.last_length[idx]), k


def test_checkpoint_round_trip_continues_bit_for_bit():
    n = 2048
    base = load_params(fps=1000, ceiling=10.3)
    kw = dict(auto_reset=True, per_drone_physics=True, stick_noise=True, noise_seed=3, track_episodes=True)
    x = DroneBatch(base, n, device=DEV, **kw)
    x.randomize_physics(77, **RANGES)
    x.reset()
    for t in range(120):
        x.step(None, return_imu=False)
    ck = x.state_dict()
    assert tuple(ck["physics"].shape) == (13, n)
    y = DroneBatch(base, n, device=DEV, **kw)
    y.load_state_dict(ck)
    assert torch.equal(x.physics[:, :n], y.physics[:, :n])
    for t in range(150):
        x.step(None, return_imu=False)
        y.step(None, return_imu=False)
    for name in ("state", "noise_state", "ep_return", "last_length", "reward", "done"):
        assert torch.equal(getattr(x, name).view(torch.uint8), getattr(y, name).view(torch.uint8)), name
    with pytest.raises(ValueError, match="physics"):
        DroneBatch(base, n, device=DEV, auto_reset=True, stick_noise=True, noise_seed=3, track_episodes=True).load_state_dict(ck)
    old = {k: v for k, v in ck.items() if k != "physics"}                    # a file without the table loads as before
    z = DroneBatch(base, n, device=DEV, auto_reset=True, stick_noise=True, noise_seed=3, track_episodes=True)
    z.load_state_dict(old)


def test_refused_combinations_raise_with_their_message():
    base = load_params(fps=1000)
    sticks = torch.zeros((256, 4), device=DEV)
    with pytest.raises(_lib.FpvError, match="fp16 state") as e:
        DroneBatch(base, 256, device=DEV, per_drone_physics=True, fp16_state=True)
    assert e.value.code == -1
    with pytest.raises(_lib.FpvError, match="drone-mode|Racer"):
        RacerBatch(None, 256, device=DEV, per_drone_physics=True)
    b = DroneBatch(base, 256, device=DEV, per_drone_physics=True, kahan_position=True)
    with pytest.raises(_lib.FpvError, match="Kahan rows") as e:
        b.step(sticks, return_imu=False)
    assert e.value.code == -1
    with pytest.raises(_lib.FpvError, match="Kahan rows"):
        b.rollout(sticks, steps=4)
    b = DroneBatch(base, 256, device=DEV, per_drone_physics=True, with_obs_aos=True)
    with pytest.raises(_lib.FpvError, match="AoS head"):
        b.step(sticks, return_imu=False)
    b = DroneBatch(base, 256, device=DEV, per_drone_physics=True)
    with pytest.raises(_lib.FpvError, match="guidance override"):
        b.step(sticks, rotation_matrix=np.eye(3, dtype=np.float32), thrust_force=5.0, return_imu=False)
    b.step(sticks, return_imu=False)                                        # the refusal left the handle usable
    L = _lib.lib()
    assert L.fpv_set_physics(b._handle, b.physics.data_ptr() + 4, b.ld) == -4 and b"16-byte" in L.fpv_last_error()
    assert L.fpv_set_physics(b._handle, b.physics.data_ptr(), b.n - 1) == -4
    _lib.check(L.fpv_set_physics(b._handle, b.physics.data_ptr(), b.ld + 4))
    with pytest.raises(_lib.FpvError, match="row stride"):
        b.step(sticks, return_imu=False)
    _lib.check(L.fpv_set_physics(b._handle, None, 0))                       # unbound: the plain kernels again
    assert b.algorithmic_bytes() == 133
    b.step(sticks, return_imu=False)


@pytest.mark.parametrize("how", ["rollout", "step_n", "graph"])
@pytest.mark.parametrize("row", ["plain", "objects", "noise", "reset_pose"])
def test_table_rows_on_the_multi_step_calls_equal_single_steps(row, how):
    """A table alone, with an object list, with stick noise and with a reset-pose table under a tight ceiling: fpv_rollout,
    fpv_step_n and fpv_rollout_graph (with stick noise or a reset source handed on to fpv_step_n) leave the bits of the same
    handle type stepped with fpv_step - 1000 drones, two calls of k = 5."""
    n, k = 1000, 5
    base = load_params(fps=1000, ceiling=10.05) if row == "reset_pose" else load_params(fps=1000)
    kw = dict(plain={}, objects={}, noise=dict(stick_noise=True, noise_seed=9), reset_pose=dict(auto_reset=True, per_drone_reset_pose=True))[row]
    objects = G10_OBJECTS if row == "objects" else None
    sets = parameter_sets(base)
    pos, vel, ypr = _poses("objects", n) if row == "objects" else _starts(n)
    a = torch.from_numpy(_acts(2 * k, n, seed=12)).to(DEV)
    (one, _), (many, _) = (_table_batch(base, n, sets, **kw) for _ in range(2))
    for b in (one, many):
        b.reset(position=pos, velocity=vel, ypr=ypr)
    resets = 0
    for t in range(2 * k):
        one.step(a[t], object_list=objects or (), return_imu=False)
        resets += int(one.done.sum())
    for c in range(2):
        many.rollout(a[c * k:(c + 1) * k], object_list=objects, **dict(rollout=dict(fused=False), step_n={}, graph=dict(graph=True))[how])
    assert one.step_counter() == many.step_counter() == 2 * k
    assert one.algorithmic_bytes() == many.algorithmic_bytes() == (185 if row == "objects" else 177)
    for name in ("state", "reward", "done", "noise_state"):
        x, y = getattr(one, name), getattr(many, name)
        assert (x is None and y is None) or torch.equal(x.view(torch.uint8), y.view(torch.uint8)), name
    assert row != "reset_pose" or resets > n // 4, "the ceiling must reset lanes in these steps"
