"""Object detections on the GPU (include/fpv_abi.h "Object detections"): the kernel against BoxDetector.evaluate - its own
lane function on the host - bit for bit on the poses read back from the batch, with a sentinel in the row padding and in the slots
it must not write; the stepper left alone; inputs no flight visits; FpvVecEnv(detector=) with partitions, auto-resets, a moving
Target and the own-target slot; the Racer; and the g22 capture of the reference on the device."""
import functools

import numpy as np
import pytest
import torch

import detect_law
import pursuit_task as PT
from fpyv_amd import _lib, load_params
from fpyv_amd.camera import Camera, DepthCamera
from fpyv_amd.detect import BoxDetector
from fpyv_amd.env import DroneBatch, FpvVecEnv, RacerBatch
from fpyv_amd.objects import Cylinder, Gate, Ground, Target

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NMAX = 300
SENTINEL = -12345.0


def _bits(a):
    a = np.ascontiguousarray(a.cpu().numpy() if torch.is_tensor(a) else a)
    return a.view(np.uint32) if a.dtype == np.float32 else a.view(np.uint8)


@functools.lru_cache(maxsize=None)
def _scene():
    """(position, ypr) of NMAX drones within 20 m of the origin at every attitude - many see only a part of what is around them.
    Computed once; read-only."""
    rng = np.random.default_rng(22)
    pos = np.stack([rng.uniform(-20, 20, NMAX), rng.uniform(-20, 20, NMAX), rng.uniform(0.3, 8.0, NMAX)], 1)
    ypr = np.stack([rng.uniform(-40, 40, NMAX), rng.uniform(-40, 40, NMAX), rng.uniform(-180, 180, NMAX)], 1)
    ypr[7] = [180.0, 0.0, 30.0]                              # inverted
    return pos.astype(np.float32), ypr.astype(np.float32)


@functools.lru_cache(maxsize=None)
def _boxes(m):
    """m boxes around the drones of the scene, a few metres a side; computed once"""
    rng = np.random.default_rng(100 + m)
    c = np.stack([rng.uniform(-25, 25, m), rng.uniform(-25, 25, m), rng.uniform(0, 8, m)], 1)
    half = rng.uniform(0.2, 4.0, (m, 3))
    return np.concatenate([c - half, c + half], 1).astype(np.float32)


def _world(m):
    """an object list and a course whose table has m slots: 8 objects and m - 8 gates beyond 8, else m objects"""
    rng = np.random.default_rng(200 + m)
    objs = [Ground(60, 4)]
    for k in range(min(m, 8) - 1):
        p = [rng.uniform(-15, 15), rng.uniform(-15, 15), 0.0]
        objs.append(Cylinder(p, rng.uniform(0.5, 1.5), rng.uniform(2, 6)) if k % 2 else Target(p[:2] + [rng.uniform(1, 6)], rng.uniform(0.3, 1.0)))
    gates = []
    for k in range(max(0, m - 8)):
        th = 2 * np.pi * k / max(1, m - 8)
        c, s = np.cos(th + 1.0), np.sin(th + 1.0)
        gates.append(Gate([14 * np.cos(th), 14 * np.sin(th), 2.0 + (k % 3)], np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]]), 2.0,
                          shape=("rectangle", "circle", "half_circle")[k % 3]))
    return objs, gates


def _batch(n, cls=DroneBatch, **kw):
    b = cls(None if cls is RacerBatch else load_params(fps=250), n, device=DEV, **kw)
    if cls is DroneBatch:
        pos, ypr = _scene()
        b.reset(position=pos[:n], ypr=ypr[:n])
    else:
        b.reset()
    return b


def _pose(b):
    s = b.state[:10, :b.n].cpu().numpy()
    return s[0:3].T.copy(), s[6:10].T.copy()


def _fill(b):
    b.box_rows.fill_(SENTINEL); b.box_depth_rows.fill_(SENTINEL); b.box_visible_rows.view(torch.uint8).fill_(0x5A)


def _check(b, want, m):
    """the three outputs equal `want` as raw bits; columns n..ld-1 and slots >= m keep the sentinel"""
    torch.cuda.synchronize()
    n = b.n
    assert b.boxes.shape == (m, 4, n) and b.box_depth.shape == (m, n) and b.box_visible.shape == (m, n)
    assert np.array_equal(_bits(b.boxes), _bits(want["boxes"])), "boxes"
    assert np.array_equal(_bits(b.box_depth), _bits(want["depth"])), "depth"
    vis = b.box_visible_rows.view(torch.uint8)[:m, :n].cpu().numpy()
    assert np.array_equal(vis, want["visible"].astype(np.uint8)), "visible"
    assert torch.all(b.box_rows[:, :, n:] == SENTINEL) and torch.all(b.box_depth_rows[:, n:] == SENTINEL)
    assert torch.all(b.box_visible_rows.view(torch.uint8)[:, n:] == 0x5A)
    assert torch.all(b.box_rows[m:] == SENTINEL) and torch.all(b.box_depth_rows[m:] == SENTINEL) and torch.all(b.box_visible_rows.view(torch.uint8)[m:] == 0x5A)


# ---- 1. bit identity ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 127, 128, 129, 300])
def test_kernel_equals_evaluate_bit_for_bit_at_every_size(n):
    """every drone count at the batch's own padded ld, every table size - one group, the group boundary, the full table"""
    for m in (1, 8, 9, 72):
        objs, gates = _world(m)
        det = BoxDetector(camera=Camera(35.0, [0.1, 0.0, 0.0], [640, 480], fov=120.0))
        b = _batch(n, gates=gates or None, detector=det, detect_slots=72)
        assert b.ld > n and b.ld % 4 == 0
        _fill(b)
        out = b.detect(objs)
        p, q = _pose(b)
        want = det.evaluate(p, q, objs, gates)
        assert want["boxes"].shape[0] == m and out.data_ptr() == b.box_rows.data_ptr()
        _check(b, want, m)
        if m == 72 and n == 300:
            assert want["visible"].any() and not want["visible"].all() and (want["depth"] == 0).any()
        b.close()


@pytest.mark.parametrize("pixels", ["int", "float"])
@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("own", [False, True])
def test_kernel_equals_evaluate_for_every_option(pixels, clip, own):
    n, m = 129, 9
    objs, gates = _world(m)
    det = BoxDetector(camera=DepthCamera(), pixels=pixels, clip=clip, own_target=own)
    kw = dict(pursuit=PT.task(targets=PT.start_targets(n))) if own else {}
    b = _batch(n, gates=gates, detector=det, detect_slots=12, **kw)
    _fill(b)
    b.detect(objs)
    p, q = _pose(b)
    if own:
        rows = b.target_position_rows[:, :n].cpu().numpy()
        rad = b.target_rows[_lib.TGT_RADIUS, :n].cpu().numpy()
        want = det.evaluate(p, q, objs, gates, target_rows=rows, target_radius=rad)
        assert np.unique(rad).size > 1 and want["visible"][m].any()
    else:
        want = det.evaluate(p, q, objs, gates)
    _check(b, want, m + int(own))
    b.close()


# ---- 2. the stepper is left alone -----------------------------------------------------------------------------------------------
def test_detect_leaves_the_state_the_step_counter_and_the_rotation_alone():
    n = 257
    objs, gates = _world(9)
    det = BoxDetector()
    with_d = _batch(n, gates=gates, detector=det)
    without = _batch(n, gates=gates)
    rot = lambda b: b.rotation            # fpv_get_rotation  # noqa: E731
    before, steps, r0 = with_d.state.clone(), with_d.step_counter(), rot(with_d)
    with_d.detect(objs)
    torch.cuda.synchronize()
    assert torch.equal(with_d.state, before) and with_d.step_counter() == steps and rot(with_d) == r0
    sticks = torch.from_numpy(np.random.default_rng(4).uniform(-0.3, 0.3, (40, n, 4)).astype(np.float32)).to(DEV)
    for t in range(40):
        with_d.step(sticks[t]); with_d.detect()
        without.step(sticks[t])
    torch.cuda.synchronize()
    assert np.array_equal(_bits(with_d.state), _bits(without.state)) and torch.equal(with_d.gate_word, without.gate_word)
    assert torch.equal(with_d.reward, without.reward) and with_d.step_counter() == without.step_counter() == 40 and rot(with_d) == rot(without)
    for b in (with_d, without):
        b.close()


# ---- 3. inputs no flight visits -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pixels", ["int", "float"])
def test_inputs_no_flight_visits_match_the_host_bit_for_bit(pixels):
    n = 16
    det = BoxDetector(camera=Camera(0.0, [0.0, 0.0, 0.0], [640, 480], fov=90.0), pixels=pixels)
    b = _batch(n, detector=det, detect_slots=8)
    st = b.state
    st[0:3, :n] = torch.tensor([[0.0], [0.0], [5.0]], device=DEV)
    st[6:10, :n] = torch.tensor([[1.0], [0.0], [0.0], [0.0]], device=DEV)          # the camera looks along +x from (0, 0, 5)
    nan, inf = float("nan"), float("inf")
    st[0, 1], st[1, 2], st[2, 3] = nan, inf, -inf                                  # NaN and Inf in the position
    st[6:10, 4] = torch.tensor([2.0, 0.0, 0.0, 0.0], device=DEV)                   # a non-unit quaternion
    st[6:10, 5] = 0.0                                                              # the zero quaternion
    st[6:10, 6] = torch.tensor([nan, 0.0, 0.0, 0.0], device=DEV)
    st[0, 7], st[6:10, 8] = 1.0e30, torch.tensor([0.3, -0.7, 2.5, 1.0e19], device=DEV)
    boxes = np.array([[-1.0, -1.0, 4.0, 1.0, 1.0, 6.0],                            # the camera inside: four corners behind
                      [-9.0, -1.0, 4.0, -7.0, 1.0, 6.0],                           # wholly behind
                      [0.0, -1.0, 4.0, 3.0, 1.0, 6.0],                             # four corners at depth exactly 0
                      [4.0, 0.5, 5.5, 4.0, 0.5, 5.5],                              # zero extent
                      [-1.0e30, -1.0e30, -1.0e30, 1.0e30, 1.0e30, 1.0e30],         # coordinates of 1e30
                      [1.0e30, 1.0e30, 1.0e30, 1.0e30, 1.0e30, 1.0e30],
                      [5.0, -2.0, 3.0, 9.0, 2.0, 7.0]], dtype=np.float32)          # an ordinary one
    t = _lib.FpvBoxes()
    t.count = len(boxes)
    for m in range(len(boxes)):
        t.box[m][:] = [float(x) for x in boxes[m]]
    import ctypes as C
    b._detect.table, b._detect_count = C.addressof(t), len(boxes)
    _fill(b)
    b._sensor_raw(b._L.fpv_detect_boxes, b._detect, None)
    p, q = _pose(b)
    want = det.evaluate(p, q, boxes=boxes)
    _check(b, want, len(boxes))
    vis = want["visible"]
    assert vis[0, 0] and vis[6, 0] and not vis[1, 0] and want["depth"][1, 0] == 0.0 and np.all(want["boxes"][1, :, 0] == 0.0)
    assert want["depth"][2, 0] == 3.0                                               # the corners at depth 0 are not in front
    assert want["depth"][3, 0] == 4.0 and want["boxes"][3, 0, 0] == want["boxes"][3, 2, 0]
    assert not vis[:, 1].any() and not vis[:, 6].any()                              # a NaN pose: visible 0
    b.close()


# ---- 4. the env -----------------------------------------------------------------------------------------------------------------
def _env(parts, every, **kw):
    objs, gates = _world(10)
    params = load_params(fps=250, ceiling=6.0)
    env = FpvVecEnv(params, num_envs=300, device=DEV, auto_reset=True, object_list=objs, gates=gates, partitions=parts,
                    detector=BoxDetector(camera=DepthCamera()), detect_every=every, **kw)
    rng = np.random.default_rng(9)
    pos = np.stack([rng.uniform(-8, 8, 300), rng.uniform(-8, 8, 300), rng.uniform(4.0, 5.9, 300)], 1).astype(np.float32)
    vel = np.stack([rng.uniform(-1, 1, 300), rng.uniform(-1, 1, 300), rng.uniform(2.0, 9.0, 300)], 1).astype(np.float32)
    env.reset(position=pos, velocity=vel)
    return env


def test_env_with_partitions_equals_the_unpartitioned_env_and_detect_every_zero_waits():
    one, two, never = _env(1, 2), _env(2, 2), _env(1, 0)
    assert two.partitions == 2 and one.boxes.shape == (10, 4, 300)
    torch.cuda.synchronize()
    assert never.boxes.shape[0] == 0 and not never.batch.box_rows.any()            # detect_every=0: not even after the reset
    sticks = torch.from_numpy(np.random.default_rng(5).uniform(-0.2, 0.2, (20, 300, 4)).astype(np.float32)).to(DEV)
    sticks[..., 3] = 0.8
    resets = 0
    for t in range(20):
        _, _, done, info = one.step(sticks[t])
        _, _, done2, info2 = two.step(sticks[t])
        never.step(sticks[t])
        torch.cuda.synchronize()
        resets += int(done.sum())
        assert torch.equal(done, done2)
        for a, b in ((one.boxes, two.boxes), (one.box_depth, two.box_depth), (one.box_visible, two.box_visible), (one.obs, two.obs)):
            assert np.array_equal(_bits(a), _bits(b)), t
        assert info["boxes"].data_ptr() == one.boxes.data_ptr() and info2["box_visible"].shape == (10, 300) and info["box_depth"].shape == (10, 300)
        if t % 2 == 1:                                                             # detected after this step: the boxes belong to obs
            s = one.batch.state[:10, :300].cpu().numpy()
            want = one.batch.detector.evaluate(s[0:3].T, s[6:10].T, one.object_list, one.batch._gate_list)
            assert np.array_equal(_bits(one.boxes), _bits(want["boxes"])) and np.array_equal(one.box_visible.cpu().numpy(), want["visible"])
    assert resets > 20 and one.box_visible.any()
    assert never.boxes.shape[0] == 0 and not never.batch.box_rows.any() and not never.batch.box_visible_rows.any()
    got = never.detect()
    torch.cuda.synchronize()
    s = never.batch.state[:10, :300].cpu().numpy()
    assert np.array_equal(_bits(got), _bits(never.batch.detector.evaluate(s[0:3].T, s[6:10].T, never.object_list, never.batch._gate_list)["boxes"]))
    for e in (one, two, never):
        e.close()


def test_a_moving_target_and_moved_gates_are_boxed_where_they_are():
    n = 64
    target = Target([6.0, 0.0, 4.0], 0.5, path=dict(radius=3.0, resolution=12))
    gates = _world(10)[1]
    det = BoxDetector(camera=DepthCamera(), pixels="float")
    env = FpvVecEnv(load_params(fps=250), num_envs=n, device=DEV, object_list=[target], gates=gates, detector=det)
    env.reset()
    a = torch.zeros((n, 4), device=DEV)
    seen = []
    for t in range(3):
        target.update()
        env.step(a)
        torch.cuda.synchronize()
        s = env.batch.state[:10, :n].cpu().numpy()
        want = det.evaluate(s[0:3].T, s[6:10].T, [target], gates)
        assert np.array_equal(_bits(env.boxes), _bits(want["boxes"]))
        seen.append(env.boxes[0].clone())
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])
    before = env.boxes[1:].clone()
    moved = [Gate(np.asarray(g.position) + [0.0, 0.0, 1.0], g.rotation_matrix, g.size, shape=g.shape) for g in gates]
    env.set_gates(moved)
    env.step(a)
    torch.cuda.synchronize()
    s = env.batch.state[:10, :n].cpu().numpy()
    want = det.evaluate(s[0:3].T, s[6:10].T, [target], moved)
    assert np.array_equal(_bits(env.boxes), _bits(want["boxes"])) and not torch.equal(env.boxes[1:], before)
    # a checkpoint holds the descriptor rows, not the gates: a batch built with other gates refuses to box the loaded course until it
    # is given the gates; one built with the same gates goes on
    d = env.batch.state_dict()
    other = DroneBatch(load_params(fps=250), n, device=DEV, gates=gates, detector=det, auto_reset=True, track_episodes=True)
    other.load_state_dict(d)
    with pytest.raises(ValueError, match="call set_gates"):
        other.detect([target])
    other.set_gates(moved)
    same = DroneBatch(load_params(fps=250), n, device=DEV, gates=moved, detector=det, auto_reset=True, track_episodes=True)
    same.load_state_dict(d)
    other.detect([target]); same.detect([target])
    torch.cuda.synchronize()
    assert np.array_equal(_bits(other.boxes), _bits(want["boxes"])) and np.array_equal(_bits(same.boxes), _bits(want["boxes"]))
    for b in (other, same):
        b.close()
    env.close()


def test_the_own_target_slot_follows_the_pursuit_task_and_the_racer_agrees_with_the_drone():
    n = 257
    det = BoxDetector(own_target=True)
    env = FpvVecEnv(load_params(fps=250), num_envs=n, device=DEV, pursuit=PT.task(targets=PT.start_targets(n)), detector=det)
    env.reset()
    a = torch.zeros((n, 4), device=DEV)
    for _ in range(3):
        env.step(a)
    torch.cuda.synchronize()
    s = env.batch.state[:10, :n].cpu().numpy()
    rows = env.target_position.t().contiguous().cpu().numpy()
    rad = env.batch.target_rows[_lib.TGT_RADIUS, :n].cpu().numpy()
    want = det.evaluate(s[0:3].T, s[6:10].T, target_rows=rows, target_radius=rad)
    assert env.boxes.shape == (1, 4, n) and np.array_equal(_bits(env.boxes), _bits(want["boxes"]))
    assert np.array_equal(env.box_visible.cpu().numpy(), want["visible"])
    with pytest.raises(ValueError, match="own_target=True"):
        DroneBatch(load_params(fps=250), 8, device=DEV, detector=det)
    env.close()
    # the Racer: the same poses, the same boxes
    objs, _ = _world(8)
    plain = BoxDetector()
    d, r = _batch(n, detector=plain), _batch(n, cls=RacerBatch, detector=plain)
    r.state[0:3, :n] = d.state[0:3, :n]; r.state[6:10, :n] = d.state[6:10, :n]
    d.detect(objs); r.detect(objs)
    torch.cuda.synchronize()
    for x, y in ((d.boxes, r.boxes), (d.box_depth, r.box_depth), (d.box_visible, r.box_visible)):
        assert np.array_equal(_bits(x), _bits(y))
    assert d.box_visible.any()
    with pytest.raises(ValueError, match="without detector="):
        _batch(8).detect(objs)
    with pytest.raises(ValueError, match="detect_slots=8"):
        _batch(8, detector=plain, detect_slots=4).detect(objs)
    for b in (d, r):
        b.close()


# ---- 5. the reference on the device ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [0, 1])
def test_the_g22_poses_on_the_device_meet_the_capture_and_the_host(c):
    cap = detect_law.load()
    objs, gates = detect_law.scene(cap)
    n = cap["p"].shape[0]
    for pixels in ("int", "float"):
        det = detect_law.detector(cap, c, pixels)
        b = DroneBatch(load_params(fps=250), n, device=DEV, gates=gates, detector=det)
        b.reset()
        b.state[0:3, :n] = torch.from_numpy(cap["p"].T.astype(np.float32)).to(DEV)
        b.state[6:10, :n] = torch.from_numpy(cap["q"].T.astype(np.float32)).to(DEV)
        b.detect(objs)
        torch.cuda.synchronize()
        got = dict(boxes=b.boxes.cpu().numpy(), depth=b.box_depth.cpu().numpy(), visible=b.box_visible.cpu().numpy())
        n_c, out_c, n_v, out_v = detect_law.check_against_capture(cap, c, pixels, got)
        assert out_c <= 0.02 * n_c and out_v <= 0.02 * n_v
        host = det.evaluate(cap["p"], cap["q"], objs, gates)
        for k in got:
            assert np.array_equal(_bits(got[k]), _bits(host[k])), k
        b.close()
