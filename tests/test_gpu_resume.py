"""Checkpoint resume of envs that carry attachments.  Env A is reset, steps K times, takes `state_dict()` - sent through torch.save and
torch.load(weights_only=True) -, and steps M more times.  Env B comes from the same factory and is made DIRTY first - reset to other
poses, four steps under other sticks, which also leaves every sensor cadence on another phase than A's (4 % 2 != 5 % 2, 4 % 3 != 5 % 3)
-, then loads the checkpoint and takes the same M steps.  After every one of them B's obs, reward, done, every `info` entry and every
public tensor of the batch equal A's BIT FOR BIT and key for key.  There is no tolerance in this module: the reference is the
uninterrupted run of the same build, which the other GPU tests hold against the host functions and the goldens.

One exception.  Checkpoints do not carry sensor outputs (DESIGN 1 "Checkpoints"): an output of a cadenced sensor - depth, boxes,
point image, centroid, lit, and their `info` entries - is compared from the first step after the load at which that sensor
launches; until then B holds what it held before.  Everything else is compared from the first step.

A moving `Target` is the caller's, not the checkpoint's: B has its own, update()d as often as A's was when the checkpoint was taken.

Every case asserts what keeps it from passing vacuously: in-kernel auto-resets in A's window after the load, a finite guidance thrust
(guided), a capture or respawn (pursuit), non-zero sensor outputs, gate events (the course of another length), and that B's state,
target rows, gate words and prev_pixel differed from A's before the load.

Option combinations the library refuses by name shape the matrix: a gate course flies neither under the guidance override nor with
Kahan rows nor with a physics table, so the guided env has no course and the step options are spread over three envs."""
import numpy as np
import pytest
import torch

import pursuit_task as PT
from attached_env import COLUMNS_LAST, DEV, N, OUTPUTS, VIEWS, bits, env as _attached, same, task_and_starts, world as _world
from fpyv_amd import _lib, load_params
from fpyv_amd.camera import DepthCamera
from fpyv_amd.env import FpvVecEnv
from fpyv_amd.objects import Cylinder, Gate, Ground
from fpyv_amd.pns import PointAndShoot
from fpyv_amd.splat import PointCloudCamera

pytestmark = pytest.mark.gpu
K, M, DIRTY = 5, 6, 4
EVERY = (2, 3, 2)                   # (depth, detect, cloud)_every: K = 5 steps after the reset leave every cadence in mid-cycle
# further public tensors of a batch, where it has them
MORE = ("state", "ep_length", "noise_state", "pos_comp", "done_bits", "physics", "reset_pose", "gate_start", "pns_prev_pixel")
# what this library's checkpoints hold that its parent's did not (case f takes them out)
NEW_KEYS = ("pursuit_rotation", "pursuit_thrust", "sensed")
# the outputs of the cadenced sensors, by the env option that sets the cadence
CADENCED = dict(depth_every=("batch/depth", "view/depth", "info/depth"),
                detect_every=("batch/box_rows", "batch/box_depth_rows", "batch/box_visible_rows", "view/boxes", "view/box_depth",
                              "view/box_visible", "info/boxes", "info/box_depth", "info/box_visible"),
                cloud_every=("batch/points_image", "batch/points_centroid", "batch/points_lit", "view/points_image", "view/points_centroid",
                             "view/points_lit", "info/points_image", "info/points_centroid"))
RAYS = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, -1.0]]


def _sticks(seed, steps=K + M, n=N):
    a = np.random.default_rng(seed).uniform(-0.2, 0.2, (steps, n, 4)).astype(np.float32)
    a[..., 3] = 0.8
    return torch.from_numpy(a).to(DEV)


def _logical(batch, t):
    """the drones' columns of a row tensor (the padding up to the row stride is nobody's)"""
    return t[..., :batch.n] if t.dim() >= 2 and t.shape[-1] == batch.ld != batch.n else t


class _Run:
    """An env, the moving Target of its world (or None) and how it is driven: "step", or "async" = step_async on every partition and
    then step_wait on every one.  `between` is called after the launches and - "async" - before any step_wait."""

    def __init__(self, env, target=None, drive="step"):
        self.env, self.target, self.drive = env, target, drive

    def step(self, action, between=None):
        """one step of every drone -> (its record: name -> array, what `between` returned)"""
        env = self.env
        if self.target is not None:
            self.target.update()
        if self.drive == "step":
            out = env.step(action)
            extra = between() if between is not None else None
        else:
            for k in range(env.partitions):
                lo, hi = env.partition_range(k)
                env.step_async(k, action[lo:hi])
            extra = between() if between is not None else None
            parts = [env.step_wait(k) for k in range(env.partitions)]
            assert all(set(p[3]) == set(parts[0][3]) for p in parts)
            info = {key: torch.cat([p[3][key] for p in parts], -1 if key in COLUMNS_LAST else 0) for key in parts[0][3]}
            out = tuple(torch.cat([p[j] for p in parts], 0) for j in range(3)) + (info,)
        return self.record(out), extra

    def record(self, out):
        env, b = self.env, self.env.batch
        torch.cuda.synchronize()
        rec = dict(obs=out[0], reward=out[1], done=out[2], **{"info/" + key: v for key, v in out[3].items()})
        for name in OUTPUTS + MORE:
            t = getattr(b, name, None)
            if t is not None:
                rec["batch/" + name] = _logical(b, t)
        for name in VIEWS:
            t = getattr(env, name, None)
            if t is not None:
                rec["view/" + name] = t
        if getattr(b, "pursuit_guidance", None) is not None:
            rec["batch/pursuit_guidance/rotation"], rec["batch/pursuit_guidance/thrust"] = b.pursuit_guidance
        if getattr(b, "_force_multiplier_pid", None) is not None:       # (the property would make one)
            rec["batch/force_multiplier_pid.state"] = _logical(b, b.force_multiplier_pid.state)
        return {key: t.detach().cpu().numpy().copy() for key, t in rec.items()}


def _first_launch(env):
    """record key -> the first step after the load (1 = the first) from which it is compared"""
    first = {}
    for option, keys in CADENCED.items():
        every = getattr(env, option)
        j = next((j for j in range(1, M + 1) if every and (K + j) % every == 0), M + 1)
        first.update({key: j for key in keys})
    return first


def _resume(tmp_path, make_a, make_b, sticks, reset_a, reset_b, dirty_sticks=None, drive_a="step", drive_b="step", b_is_reset=True,
            strip=(), only=None, hooks=None):
    """The run of the module's docstring.  make_x() -> (env, its moving Target or None); reset_x: the keywords of env.reset();
    hooks: step index -> f(env), called on A before that step; strip: checkpoint keys taken out before the load; only: the record
    keys compared (None = all).  Returns (mismatches as (step after the load, key), figures of A's run)."""
    env_a, target_a = make_a()
    a = _Run(env_a, target_a, drive_a)
    env_a.reset(**reset_a)
    for t in range(K):
        if hooks and t in hooks:
            hooks[t](env_a)
        at_ck, ck = a.step(sticks[t], env_a.state_dict if t == K - 1 else None)
    torch.save(ck, tmp_path / "ck.pt")
    ck = torch.load(tmp_path / "ck.pt", weights_only=True)              # everything in a checkpoint survives this
    recs_a = [a.step(sticks[K + j])[0] for j in range(M)]
    first = _first_launch(env_a)
    env_a.close()

    env_b, target_b = make_b()
    b = _Run(env_b, target_b, drive_b)
    loaded = {k: v for k, v in ck.items() if k not in strip}

    def load():
        mine = env_b.state_dict()
        differ = {k: not same(mine[k], ck[k]) for k in ("state", "target_rows", "gate_word", "pns_prev_pixel") if k in ck}
        env_b.load_state_dict(loaded)
        return differ
    if b_is_reset:
        env_b.reset(**reset_b)
        for t in range(DIRTY):
            _, differ = b.step(dirty_sticks[t], load if t == DIRTY - 1 else None)
        assert all(differ.values()), f"B was not dirty before the load: {differ}"
        for option in CADENCED:
            every = getattr(env_b, option)
            assert every in (0, 1) or DIRTY % every != K % every, option
    else:
        load()
    if target_b is not None:
        for _ in range(K - (DIRTY if b_is_reset else 0)):
            target_b.update()
    recs_b = [b.step(sticks[K + j])[0] for j in range(M)]
    env_b.close()

    bad = []
    for j, (ra, rb) in enumerate(zip(recs_a, recs_b), 1):
        if set(ra) != set(rb):
            bad.append((j, "keys: " + " ".join(sorted(set(ra) ^ set(rb)))))
        for key in sorted(set(ra) & set(rb)):
            if (only is None or key in only) and j >= first.get(key, 1) and not same(ra[key], rb[key]):
                bad.append((j, key))
    spawns = [r["batch/target_rows"].view(np.uint32)[_lib.TGT_SPAWNS] for r in [at_ck] + recs_a if "batch/target_rows" in r]
    last = recs_a[-1]
    fig = dict(resets=[int(r["done"].sum()) for r in recs_a],
               finite=[int(np.isfinite(r["batch/pursuit_guidance/thrust"]).sum()) for r in [at_ck] + recs_a if "batch/pursuit_guidance/thrust" in r],
               respawns=int(sum((x != spawns[0]).any() for x in spawns[1:])),
               captures=int(sum(r["batch/target_event_u8"].sum() for r in recs_a if "batch/target_event_u8" in r)),
               gate_events=int(sum((r["info/gate_event"] != 0).sum() for r in recs_a if "info/gate_event" in r)),
               nonzero={key: bool(bits(last[key]).any()) for key in ("batch/range_rows",) + sum(CADENCED.values(), ()) if key in last},
               keys=len(last), first={key: j for key, j in first.items() if key in last and j > 1})
    print("\nresume:", fig, "\nmismatches (step after the load, key):", bad)
    return bad, fig


def _auto_resets(fig):
    assert sum(fig["resets"]) >= 1, fig["resets"]          # an in-kernel auto-reset in A's window after the load


# ---- a: everything attached; b: guided ---------------------------------------------------------------------------------------
def _through_gate_0(pos, vel, drones):
    """the start of `drones`: 3 cm in front of the first gate of the attachments env, flying through it at 5 m/s (the second step)"""
    pos, vel = pos.copy(), vel.copy()
    pos[drones], vel[drones] = (8.97, -3.0, 3.0), (5.0, 0.0, 0.0)
    return pos, vel


def _everything(parts, **kw):
    def make():
        objs, target = _world()
        return _attached(objs, parts, every=EVERY, **kw)[0], target
    return make


def _attached_starts(gates=True):
    """(A's reset keywords, B's - other poses)"""
    _, pos, vel = task_and_starts()
    rng = np.random.default_rng(32)
    other = (pos + rng.uniform(-0.05, 0.05, pos.shape)).astype(np.float32), (vel * rng.uniform(0.5, 1.0, vel.shape)).astype(np.float32)
    mine = (pos, vel)
    if gates:           # some drones of either partition pass a gate before the checkpoint, others in B: the gate words are not all zero
        mine, other = _through_gate_0(pos, vel, [3, 4, 5, 140, 141, 142]), _through_gate_0(*other, [10, 11, 200, 201])
    return dict(position=mine[0], velocity=mine[1]), dict(position=other[0], velocity=other[1])


@pytest.mark.parametrize("a,b", [((1, "step"), (1, "step")), ((2, "step"), (2, "step")), ((2, "async"), (2, "async")),
                                 ((1, "step"), (2, "step")), ((2, "step"), (1, "step"))],
                         ids=["one", "two", "split_phase", "one_into_two", "two_into_one"])
def test_everything_attached_resumes_bit_for_bit(tmp_path, a, b):
    reset_a, reset_b = _attached_starts()
    bad, fig = _resume(tmp_path, _everything(a[0]), _everything(b[0]), _sticks(5), reset_a, reset_b, _sticks(6), drive_a=a[1], drive_b=b[1])
    assert not bad, bad
    _auto_resets(fig)
    assert fig["respawns"] + fig["captures"] >= 1 and all(fig["nonzero"].values()) and len(fig["nonzero"]) == 1 + sum(map(len, CADENCED.values())), fig


@pytest.mark.parametrize("parts", [1, 2])
@pytest.mark.parametrize("b_is_reset", [True, False], ids=["dirty", "never_reset"])
def test_guided_env_resumes_bit_for_bit(tmp_path, parts, b_is_reset):
    reset_a, reset_b = _attached_starts(gates=False)
    make = _everything(parts, gates=False, guided=True)
    bad, fig = _resume(tmp_path, make, make, _sticks(5), reset_a, reset_b, _sticks(6), b_is_reset=b_is_reset)
    assert not bad, bad
    _auto_resets(fig)
    assert len(fig["finite"]) == 1 + M and min(fig["finite"]) >= 1 and fig["respawns"] + fig["captures"] >= 1, fig


# ---- c: point and shoot as the env's action --------------------------------------------------------------------------------------
def _assist_scene(seed):
    """tests/test_gpu_pns.py's scene: climbing starts under the ceiling, a standing target of its own ahead of and above every drone"""
    rng = np.random.default_rng(seed)
    pos = np.stack([rng.uniform(-5, 5, N), rng.uniform(-5, 5, N), rng.uniform(9.0, 10.1, N)], axis=1).astype(np.float32)
    vel = np.stack([rng.uniform(-1, 1, N), rng.uniform(-1, 1, N), rng.uniform(0.5, 8.0, N)], axis=1).astype(np.float32)
    centre = pos + np.stack([rng.uniform(6, 9, N), rng.uniform(-2, 2, N), rng.uniform(2, 5, N)], axis=1).astype(np.float32)
    return pos, vel, dict(centre=centre, radius=0.5, path_radius=0.0)


def test_assist_env_resumes_bit_for_bit_across_auto_resets(tmp_path):
    params = load_params(fps=250, ceiling=10.2)
    pos, vel, targets = _assist_scene(8)
    pos_b, vel_b, _ = _assist_scene(9)

    def make():
        law = PointAndShoot(params, ref_frame="drone", mode="frontarget", max_depth=20.0)
        return FpvVecEnv(params, num_envs=N, device=DEV, auto_reset=True, pursuit=PT.task(targets=targets, respawn_on_done=False), assist=law,
                         assist_sticks=(0.0, 0.0, 0.0, -0.646)), None
    commands = [torch.from_numpy(np.random.default_rng(s).uniform(-0.4, 0.4, (K + M, N, 4)).astype(np.float32)).to(DEV) for s in (5, 6)]
    bad, fig = _resume(tmp_path, make, make, commands[0], dict(position=pos, velocity=vel), dict(position=pos_b, velocity=vel_b), commands[1])
    assert not bad, bad
    _auto_resets(fig)
    assert fig["keys"] > 20, fig


# ---- d: a course of another length -------------------------------------------------------------------------------------------------
def _course():
    """three gates 8 cm apart across the drones' way: +x is every gate's normal, the opening 2 m wide"""
    return [Gate([x, 0.0, 3.0], np.eye(3), 2.0, shape="rectangle") for x in (0.02, 0.10, 0.18)]


def _course_starts(seed, shift=0.0):
    """up to 30 cm in front of the first gate, flying +x at 4..8 m/s (1.6..3.2 cm a step): in every step some drones cross the plane
    of their next gate, about a quarter of them beside the opening (a MISS, which ends the episode with miss_is_done)"""
    rng = np.random.default_rng(seed)
    pos = np.stack([rng.uniform(-0.3, 0.0, N) + shift, rng.uniform(-1.4, 1.4, N), 3.0 + rng.uniform(-0.6, 0.6, N)], 1).astype(np.float32)
    vel = np.stack([rng.uniform(4.0, 8.0, N), np.zeros(N), np.zeros(N)], 1).astype(np.float32)
    return dict(position=pos, velocity=vel)


def _course_env(parts, **kw):
    return FpvVecEnv(load_params(fps=250, ceiling=6.0), num_envs=N, device=DEV, auto_reset=True, partitions=parts, object_list=[Ground(40, 24)],
                     gates=_course(), miss_is_done=True, range_rays=RAYS, depth_camera=DepthCamera(resolution=(8, 4)), depth_every=2, **kw)


def test_a_checkpoint_whose_course_has_another_length_resumes_in_a_partitioned_env(tmp_path):
    hooks = {2: lambda e: e.set_gates(_course()[1:])}                   # A flies on with two of the three gates
    bad, fig = _resume(tmp_path, lambda: (_course_env(1), None), lambda: (_course_env(2), None), _sticks(5), _course_starts(1),
                       _course_starts(2, shift=-0.05), _sticks(6), hooks=hooks)
    assert not bad, bad
    _auto_resets(fig)
    assert fig["gate_events"] >= 1 and fig["nonzero"]["batch/depth"], fig


# ---- e: the step options that own state, under partitions; a Racer ------------------------------------------------------------------
JITTER = dict(reset_position_range=[[-0.5, -0.5, -0.05], [0.5, 0.5, 0.05]], reset_velocity_range=[[-0.2, -0.2, 0.0], [0.2, 0.2, 0.5]],
              reset_ypr_range_deg=[[-15.0, -15.0, -180.0], [15.0, 15.0, 180.0]], reset_seed=0xC0FFEE_1234)


def _option_env(which, other):
    """`other`: B's env, whose tables are others than A's until the load.  The library refuses Kahan rows with a physics table or a
    course, and a table with a course: three envs carry the six options between them."""
    kw = dict(num_envs=N, device=DEV, auto_reset=True, partitions=2, object_list=[Ground(40, 24), Cylinder([4.0, 3.0, 0.0], 1.0, 5.0, 17, 9)],
              range_rays=RAYS, with_done_bits=True)
    if which == "kahan":
        return FpvVecEnv(load_params(fps=250, ceiling=6.0, **JITTER), stick_noise=True, noise_seed=3, kahan_position=True, per_drone_reset_pose=True, **kw)
    if which == "physics":
        e = FpvVecEnv(load_params(fps=250, ceiling=6.0), stick_noise=True, noise_seed=3, per_drone_physics=True, **kw)
        e.randomize_physics(78 if other else 77, mass=(0.8, 1.25), thrust=(0.9, 1.1), drag=(0.5, 2.0))
        return e
    start = np.random.default_rng(4 + other).integers(0, 3, N)
    return FpvVecEnv(load_params(fps=250, ceiling=6.0), gates=_course(), gate_start=start, miss_is_done=True, per_drone_reset_pose=True, **kw)


@pytest.mark.parametrize("which", ["kahan", "physics", "gate_start"])
def test_step_options_that_own_state_resume_under_partitions(tmp_path, which):
    if which == "gate_start":
        reset_a, reset_b = _course_starts(1), _course_starts(2, shift=-0.05)
    else:
        reset_a, reset_b = _attached_starts(gates=False)
    bad, fig = _resume(tmp_path, lambda: (_option_env(which, 0), None), lambda: (_option_env(which, 1), None), _sticks(5), reset_a, reset_b, _sticks(6))
    assert not bad, bad
    _auto_resets(fig)
    assert fig["nonzero"]["batch/range_rows"] and (which != "gate_start" or fig["gate_events"] >= 1), fig


def test_racer_env_resumes_bit_for_bit(tmp_path):
    """A Racer sees a world it does not collide with: range rays, the depth camera and the point-cloud camera, no object list (an env
    binds its list to the steps, which a Racer refuses) - so the sensors see an empty world and their outputs do not depend on the
    pose: what this case holds is the Racer's state, reward, done and episode rows under partitions.  A 0.1 mm ceiling: whatever its
    thrust, a Racer leaves it within a few steps, again and again."""
    pid = np.array([[0.004, 0.02, 1e-6], [0.003, 0.01, 2e-6], [0.002, 0.005, 0]])
    params = load_params(fps=1000).replace(mode=1, racer_pid=pid, ceiling=1e-4)

    def make():
        return FpvVecEnv(params, num_envs=N, device=DEV, mode="racer", auto_reset=True, partitions=2, range_rays=RAYS, depth_camera=DepthCamera(resolution=(8, 4)),
                         cloud_camera=PointCloudCamera(resolution=(8, 4), centroid=True), depth_every=2, cloud_every=2), None

    def actions(seed):
        rng = np.random.default_rng(seed)
        a = np.concatenate([rng.uniform(-2, 2, (K + M, N, 3)), np.broadcast_to(rng.uniform(0.0, 14.0, (1, N, 1)), (K + M, N, 1))], -1)
        return torch.from_numpy(a.astype(np.float32)).to(DEV)
    bad, fig = _resume(tmp_path, make, make, actions(5), {}, {}, actions(6))
    assert not bad, bad
    _auto_resets(fig)
    assert fig["nonzero"]["batch/depth"], fig


# ---- f: a checkpoint of the parent library ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("parts", [1, 2])
def test_a_checkpoint_without_the_new_keys_loads_and_continues(tmp_path, parts):
    """all cadences 1 and no guided=: what the parent library's load continued correctly, this one continues alike"""
    def make():
        objs, target = _world()
        return _attached(objs, parts, every=(1, 1, 1))[0], target
    reset_a, reset_b = _attached_starts()
    bad, fig = _resume(tmp_path, make, make, _sticks(5), reset_a, reset_b, _sticks(6), strip=NEW_KEYS,
                       only=("obs", "reward", "done", "batch/state"))
    assert not bad, bad
    _auto_resets(fig)


def test_partitions_on_different_cadence_phases_load_only_into_as_many_partitions():
    """step_async on one partition alone leaves the two on different phases: no one count for an env of another partition number"""
    reset_a, _ = _attached_starts()
    (split, _), (one, _), (other, _) = _everything(2)(), _everything(1)(), _everything(2)()
    split.reset(**reset_a)
    lo, hi = split.partition_range(0)
    split.step_async(0, _sticks(5, 1)[0, lo:hi])
    ck = split.state_dict()
    assert ck["sensed"] == [1, 0]
    with pytest.raises(ValueError, match="'sensed'.*2 partitions"):
        one.load_state_dict(ck)
    other.load_state_dict(ck)
    assert other.state_dict()["sensed"] == [1, 0]
    for e in (split, one, other):
        e.close()
