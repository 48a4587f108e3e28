"""The flights and host expectations that tests/test_call_inputs_host.py (CPU) and tests/test_gpu_call_inputs.py share: the per-call
inputs of a step - the wind, the stick layout, the rows a step only writes - on every step-kernel family.

Every flight is defined for N = 1000 drones; a test of n drones flies the first n of them (starts, sticks and, on a table handle,
the round-robin deal of the eight airframes are prefixes), so what the CPU module asserts for 1000 drones holds for every smaller
population the GPU module uses.  The expectations are the host lane model's (oracle/lane_model.py), stepped one step at a time so
that the per-step rewards, dones and accel rows, the reset sources and the race of a gate course can be followed on the host.
"""
import ctypes as C
import functools

import numpy as np

import gate_course as gc
from conftest import load_golden
from fpyv_amd import _lib, load_params
from fpyv_amd import gates as G
from oracle import lane_model, oracle
from parity import soa_vs_oracle
from physics_sets import parameter_sets

WIND, CALM = (1.0, -2.0, 0.5), (0.0, 0.0, 0.0)        # three distinct non-zero components: no swap and no dropped one cancels
SIZES = (1, 63, 129, 1000)                            # one lane; odd inside a wave; a dead second wave; a ragged multi-block grid
N, STEPS = 1000, 300
# 400 steps per second: 300 steps are 0.75 s of flight, in which this wind moves every drone by more than 100 x the 1e-5 bar
# (measured: at 1 kHz the same 300 steps move the least-moved drone by 0.06 % of |p|, below it; at 500 per second the airframe with
# the least drag reaches 0.099 %, at 400 per second 0.15 %)
FPS = 400
G10_OBJECTS = [(2, 1.5, -6.0, 3.0, 0.8, 0.0), (1, 3.0, 0.0, 0.0, 1.0, 5.0), (1, -2.0, 2.5, 0.0, 0.6, 1.5), (0, 0.0, 0.0, 0.0, 0.0, 0.0)]
JIT = dict(reset_position_range=[[-0.5, -0.5, -0.05], [0.5, 0.5, 0.05]], reset_velocity_range=[[-0.2, -0.2, 0.0], [0.2, 0.2, 0.5]],
           reset_ypr_range_deg=[[-15.0, -15.0, -180.0], [15.0, 15.0, 180.0]], reset_seed=0xC0FFEE_1234)
CEILING = 10.2
# fp16 storage holds 4e-3 of |p|, so the wind needs a longer flight to show: 300 steps at 120 per second are 2.5 s, in which it moves
# every drone by more than 1.7 m (at 60 per second the lane model's own error against the oracle comes within a factor 3 of the bar)
FPS_FP16 = 120
GATE_CEILING = 11.0                                   # above every gate start (10 +- 0.9 m): the even lanes climb through it, the odd ones get no throttle
GATE_OBJECTS_OFFSET = np.array([1.0, 0.0, -8.0])
NOISE_SEED = 9


def sticks(steps=STEPS, n=N, seed=21):
    """tests/test_gpu_physics.py::_acts: uniform rates, throttle 0.1 +- 0.4"""
    return gc.acts(steps, n, seed)


def soa_sticks(n):
    """[n, 4] sticks whose four channels differ for every drone (EMA noise plus an offset per channel): a wrong row stride, a wrong
    channel or a wrong lane shows in the first step"""
    from fpyv_amd import sticks as S
    return (S.ema_noise(8, range(n), seed=3)[-1] + np.array([0.11, -0.23, 0.31, 0.17])).astype(np.float32)


def _starts(name):
    rng = np.random.default_rng(5)
    n = N
    if name == "ground":                    # tests/test_gpu_physics.py::_poses: sinking onto the ground plane
        pos = np.stack([rng.uniform(-3, 3, n), rng.uniform(-3, 3, n), rng.uniform(0.03, 0.14, n)], 1)
        vel = np.stack([rng.uniform(-1, 1, n), rng.uniform(-1, 1, n), rng.uniform(-1.5, 0.0, n)], 1)
        return pos, vel, rng.uniform(-8, 8, (n, 3))
    if name == "objects":                   # the G10 capture's starts, tiled
        g = load_golden("g10_objects")
        k = np.arange(n) % g["init_position"].shape[0]
        return g["init_position"][k], g["init_velocity"][k], g["init_ypr"][k]
    if name == "gates":
        return gc.starts(n)
    if name == "ceiling":                   # just below the ceiling: the even lanes climb through it again and again, the odd ones start 5 m lower, diving, and never reach it
        up = (np.arange(n) % 2 == 0)
        pos = np.stack([rng.uniform(-5, 5, n), rng.uniform(-5, 5, n), np.where(up, rng.uniform(10.0, 10.1, n), rng.uniform(5.0, 5.1, n))], 1)
        vel = np.stack([rng.uniform(-1, 1, n), rng.uniform(-1, 1, n), np.where(up, rng.uniform(1.5, 4.0, n), rng.uniform(-8.0, -6.0, n))], 1)
        return pos.astype(np.float32), vel.astype(np.float32), rng.uniform(-20, 20, (n, 3)).astype(np.float32)
    pos = np.stack([rng.uniform(-3, 3, n), rng.uniform(-3, 3, n), 10.0 + rng.uniform(-0.9, 0.9, n)], 1)
    vel = np.stack([rng.uniform(-2, 2, n), rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)], 1)
    return pos, vel, rng.uniform(-8, 8, (n, 3))


@functools.lru_cache(maxsize=None)
def flight(name):
    """dict(p, pos, vel, ypr, init [14, N], acts [STEPS, N, 4], objects) of a named flight; read-only"""
    kw = dict(plain={}, objects={}, gates={}, gates_objects={}, gates_ceiling=dict(ceiling=GATE_CEILING), ground=dict(ground=True, ground_damping=2.0),
              ceiling=dict(ceiling=CEILING), jitter=dict(ceiling=CEILING, **JIT), fp16={})[name]
    p = load_params(fps=FPS_FP16 if name == "fp16" else FPS, **kw)
    pos, vel, ypr = _starts(dict(jitter="ceiling", gates_objects="gates", gates_ceiling="gates", fp16="plain").get(name, name))
    if name == "gates_objects":             # tests/test_gpu_gates.py: the course and the starts moved next to the G10 list's cylinder
        pos = pos + GATE_OBJECTS_OFFSET
    init = np.ascontiguousarray(lane_model.initial_state(p, N, pos, vel, ypr, as_reset_kernel=name in ("ceiling", "jitter", "gates_ceiling"))[:, :N])
    a = sticks()
    if name == "gates_ceiling":
        a[:, 1::2, 3] = np.float32(-0.9)              # (next to no thrust: they sink)
    for x in (init, a):
        x.setflags(write=False)
    return dict(p=p, pos=pos, vel=vel, ypr=ypr, init=init, acts=a, objects=tuple(G10_OBJECTS) if name in ("objects", "gates_objects") else ())


def init_pose(p):
    """[10] float32: init_position / init_velocity / init_quat as fpv_create narrows them - what the in-kernel auto-reset without a
    reset source puts into a lane (fpyv_amd.env._Batch._init_pose)"""
    c = _lib.pack_params(p, auto_reset=True)
    q = [float(c.init_quat[k]) for k in range(4)]
    qn = (q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]) ** 0.5
    return np.array(list(c.init_position) + list(c.init_velocity) + [x / qn for x in q], dtype=np.float32)


def reset_sample(cp, gid, step, base):
    """fpv_reset_pose_sample: the pose an in-kernel reset (e = 0) of global drone `gid` at step `step` takes from `base` [10]"""
    b = np.ascontiguousarray(base, dtype=np.float32)
    out = np.empty(10, dtype=np.float32)
    assert _lib.lib().fpv_reset_pose_sample(C.byref(cp), int(gid), int(step), 0, b.ctypes.data, out.ctypes.data) == 0
    return out


def noise_sticks(p, acts, n, seed=NOISE_SEED, drone_id_offset=0, step0=0):
    """(applied [k, n, 4], noise_state [4, n]): the sticks a noise handle applies on top of `acts` (None: pure noise, k = STEPS)"""
    k = STEPS if acts is None else acts.shape[0]
    applied, ns = lane_model.stick_noise(p, n, k, noise_seed=seed, drone_id_offset=drone_id_offset,
                                         base_actions=None if acts is None else np.ascontiguousarray(acts[:, :n]), step0=step0)
    return applied, ns[:, :n]


def fly(p, init, acts, wind=WIND, objects=(), kahan=False, override=None, auto_reset=False, reset=None):
    """The host lane model, one step at a time, from init [14, n] under acts [k, n, 4].  `override` = (R [n, 3, 3], f [k, n]);
    `auto_reset` = the lane model's own reset to init_*; `reset` = dict(cp, base [10, n], gid [n], step0): a reset source - the lane
    that is done takes fpv_reset_pose_sample's pose for its global id.  Returns dict(snaps [k + 1, 14, n], accel [k, 3, n], done [k, n] bool,
    reward [k, n], comp [6, n] or None)."""
    k, n = acts.shape[:2]
    s = np.ascontiguousarray(init[:, :n], dtype=np.float32).copy()
    comp = np.zeros((6, n), np.float32) if kahan else None
    snaps, accel = np.empty((k + 1, 14, n), np.float32), np.empty((k, 3, n), np.float32)
    done, reward = np.zeros((k, n), bool), np.empty((k, n), np.float32)
    snaps[0] = s
    try:
        lane_model.set_objects(tuple(objects))
        lane_model.set_pos_comp(comp)
        for t in range(k):
            if override is not None:
                lane_model.set_override(override[0], override[1][t])
            _, acc, d, r = lane_model.run(p, s, np.ascontiguousarray(acts[t:t + 1, :n]), wind=wind, n=n, auto_reset=auto_reset and reset is None)
            accel[t], done[t], reward[t] = acc[:, :n], d.astype(bool), r
            if reset is not None:
                for i in np.flatnonzero(d):
                    s[0:10, i] = reset_sample(reset["cp"], reset["gid"][i], reset["step0"] + t, reset["base"][:, i])
                    s[10:14, i] = 0.0
                    if comp is not None:
                        comp[:, i] = 0.0
            snaps[t + 1] = s
    finally:
        lane_model.set_objects(())
        lane_model.set_pos_comp(None)
        lane_model.set_override(None)
    return dict(snaps=snaps, accel=accel, done=done, reward=reward, comp=comp)


def fly_table(sets, init, acts, **kw):
    """`fly` with the eight airframes dealt round-robin (physics_sets.dealt): one lane-model run per set on that set's columns"""
    k, n = acts.shape[:2]
    which = np.arange(n) % len(sets)
    out = dict(snaps=np.empty((k + 1, 14, n), np.float32), accel=np.empty((k, 3, n), np.float32), done=np.zeros((k, n), bool),
               reward=np.empty((k, n), np.float32), comp=None)
    reset = kw.pop("reset", None)
    for j, p in enumerate(sets):
        idx = np.flatnonzero(which == j)
        if idx.size == 0:
            continue
        r = None if reset is None else dict(reset, base=np.ascontiguousarray(reset["base"][:, idx]), gid=np.asarray(reset["gid"])[idx])
        e = fly(p, np.ascontiguousarray(init[:, idx]), np.ascontiguousarray(acts[:, idx]), reset=r, **kw)
        for name in ("snaps", "accel", "done", "reward"):
            out[name][..., idx] = e[name]
    return out


def fly_gates(p, init, acts, rows, wind=WIND, objects=(), auto_reset=False, reset=None, **course):
    """The race of a gate handle on the host: the lane model's step, then fpv_gate_eval (fpyv_amd.gates.evaluate) on the position the
    step started from and the one it produced; with `auto_reset` a lane whose episode ends - by the physics or by the race - goes
    back to init_* - with `reset` (see `fly`) to the pose of its reset source - and its word to its start gate.  `course`: laps,
    gate_rewards, miss_is_done, gate_start.  Returns `fly`'s dict
    (done and reward are the race's) and words [k, n] uint32, obs [k, n, 6], phys_done [k, n]."""
    k, n = acts.shape[:2]
    s = np.ascontiguousarray(init[:, :n], dtype=np.float32).copy()
    start = course.get("gate_start")
    word = np.zeros(n, np.uint32) if start is None else np.asarray(start, np.uint32)[:n].copy()
    pose = init_pose(p)
    out = dict(snaps=np.empty((k + 1, 14, n), np.float32), accel=np.empty((k, 3, n), np.float32), done=np.zeros((k, n), bool),
               reward=np.empty((k, n), np.float32), words=np.empty((k, n), np.uint32), obs=np.empty((k, n, 6), np.float32),
               phys_done=np.zeros((k, n), bool), comp=None)
    out["snaps"][0] = s
    try:
        lane_model.set_objects(tuple(objects))
        for t in range(k):
            po = s[0:3].T.copy()
            _, acc, d, _ = lane_model.run(p, s, np.ascontiguousarray(acts[t:t + 1, :n]), wind=wind, n=n)
            pn, qn = s[0:3].T.copy(), s[6:10].T.copy()
            w, r, dn, ob = G.evaluate(rows, po, pn, qn, d, word, **course)
            if auto_reset and dn.any():
                for i in np.flatnonzero(dn):
                    s[0:10, i] = pose if reset is None else reset_sample(reset["cp"], reset["gid"][i], reset["step0"] + t, reset["base"][:, i])
                s[10:14, dn] = 0.0
                w, r, dn, ob = G.evaluate(rows, po, pn, qn, d, word, auto_reset=True, p_after=s[0:3].T.copy(), q_after=s[6:10].T.copy(), **course)
            word = w
            out["snaps"][t + 1], out["accel"][t], out["phys_done"][t] = s, acc[:, :n], d.astype(bool)
            out["words"][t], out["reward"][t], out["done"][t], out["obs"][t] = w, r, dn, ob
    finally:
        lane_model.set_objects(())
    return out


def drift(e_wind, e_calm, lanes=None):
    """min over the drones of |p_wind - p_calm| / |p_wind| at the end of the two flights: the wind's effect in the measure the
    parity bar uses (parity.soa_vs_oracle pos_rel)"""
    a, b = e_wind["snaps"][-1][0:3].astype(np.float64), e_calm["snaps"][-1][0:3].astype(np.float64)
    d = np.linalg.norm(a - b, axis=0) / np.linalg.norm(a, axis=0)
    return float((d if lanes is None else d[lanes]).min())


def episode_rows(rewards, dones):
    """(ep_return, ep_length, last_return, last_length) after per-step rewards [k, n] and dones [k, n] from zeroed rows: float32
    adds in step order, zeroed on done, last_* taken at the done (csrc/fpv_kernels.h emit_lane_outputs / RollOut)"""
    k, n = rewards.shape
    ep_r, ep_l = np.zeros(n, np.float32), np.zeros(n, np.int32)
    last_r, last_l = np.zeros(n, np.float32), np.zeros(n, np.int32)
    for t in range(k):
        ep_r = (ep_r + rewards[t].astype(np.float32)).astype(np.float32)
        ep_l = ep_l + 1
        d = dones[t].astype(bool)
        last_r, last_l = np.where(d, ep_r, last_r), np.where(d, ep_l, last_l)
        ep_r, ep_l = np.where(d, np.float32(0), ep_r).astype(np.float32), np.where(d, 0, ep_l).astype(np.int32)
    return ep_r, ep_l, last_r.astype(np.float32), last_l.astype(np.int32)


def unpack_bits(words, n):
    """[..., ceil(n / 64)] int64 done-bit words -> [..., n] bool"""
    w = np.ascontiguousarray(words).view(np.uint64)
    return (((w[..., None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).reshape(w.shape[:-1] + (-1,))[..., :n]).astype(bool)


_SETS = {}


def table_sets(p):
    """the eight airframes of tests/physics_sets.py on base parameters `p`, built once per base"""
    if id(p) not in _SETS:
        _SETS[id(p)] = (p, tuple(parameter_sets(p)))
    return _SETS[id(p)][1]


def override_inputs(n, steps=STEPS):
    """(R [n, 3, 3] float32, f [steps, n] float32) of a guidance call per step: an attitude a few degrees off level per drone,
    thrust forces around the weight, NaN (= not overridden) for a third of the drone-steps"""
    rng = np.random.default_rng(13)
    y, p, r = np.deg2rad(rng.uniform(-12, 12, (3, N)))
    cy, sy, cp, sp, cr, sr = np.cos(y), np.sin(y), np.cos(p), np.sin(p), np.cos(r), np.sin(r)
    R = np.stack([cy * cp, cy * sp * sr - sy * cr, cy * sp * cr + sy * sr, sy * cp, sy * sp * sr + cy * cr, sy * sp * cr - cy * sr,
                  -sp, cp * sr, cp * cr], axis=1).reshape(N, 3, 3).astype(np.float32)
    f = rng.uniform(5.0, 12.0, (steps, N)).astype(np.float32)
    f[rng.random((steps, N)) < 1 / 3] = np.nan
    return np.ascontiguousarray(R[:n]), np.ascontiguousarray(f[:, :n])


# ---- the rows of the wind table: a key, the host flight of 1000 drones under it, the float64 oracle's end of the same flight ----
# ("plain", noise, obj, kahan)   the eight plain instantiations          ("override", obj)    the guidance-override kernels
# ("table", noise, world)        world: plain | ground | objects         ("gate", variant)    plain | noise | objects | reset
# ("reset", jitter)              the reset-source route                   ("fp16",)            fp16 storage (see `host_h`)
# outside the table: ("table_reset",) a table handle with a reset source, ("gate", "finish") a one-lap course under a ceiling,
# ("book", row) the row's flight on a handle that resets its lanes to init_* under a ceiling (the bookkeeping tests)
def reset_source(p, init, n=N, drone_id_offset=0):
    return dict(cp=_lib.pack_params(p, auto_reset=True, drone_id_offset=drone_id_offset), base=np.ascontiguousarray(init[0:10, :n]),
                gid=drone_id_offset + np.arange(n), step0=0)


BOOK_CEILING = 10.6
_BOOK = {}


def row_flight(row):
    kind = row[0]
    if kind == "book":                      # the row's flight under a ceiling (its own, or one 0.6 m above init_position)
        if row not in _BOOK:
            fl = row_flight(row[1])
            _BOOK[row] = fl if np.isfinite(fl["p"].ceiling) else dict(fl, p=fl["p"].replace(ceiling=BOOK_CEILING))
        return _BOOK[row]
    if kind == "plain":
        return flight("objects" if row[2] else "plain")
    if kind == "override":
        return flight("objects" if row[1] else "plain")
    if kind == "table":
        return flight(row[2])
    if kind == "gate":
        return flight(dict(plain="gates", noise="gates", objects="gates_objects", reset="gates_ceiling", finish="gates_ceiling")[row[1]])
    if kind == "table_reset":
        return flight("ceiling")
    if kind == "reset":
        return flight("jitter" if row[1] else "ceiling")
    return flight("fp16")


def gate_rows(row):
    """[4, 16] descriptor rows of the row's course (tests/gate_course.py; moved with the starts next to the cylinder for `objects`)"""
    course = gc.course()
    if row[1] == "objects":
        for g in course:
            g.position = g.position + GATE_OBJECTS_OFFSET
    return course, G.derive(course)


def fly_row(row, acts=None, n=N, wind=WIND, auto_reset=False):
    """The host flight of the row's first n drones under `acts` [k, n, 4] (None: the flight's own 300 steps): `fly`'s dict, and
    `acts`: the sticks applied - with stick noise the generator's output on top of the given ones -, `ns`: the noise rows after the
    flight.  `auto_reset`: the handle resets lanes to init_* (rows without a reset source)."""
    fl = row_flight(row)
    if row[0] == "book":
        row, auto_reset = row[1], True
    kind = row[0]
    p, init, ns = fl["p"], fl["init"][:, :n], None
    acts = fl["acts"][:, :n] if acts is None else acts
    k = acts.shape[0]
    noise = (kind in ("plain", "table") and row[1]) or (kind == "gate" and row[1] == "noise")
    if noise:
        acts, ns = noise_sticks(p, acts, n)
    if kind == "plain":
        e = fly(p, init, acts, wind, objects=fl["objects"], kahan=bool(row[3]), auto_reset=auto_reset)
    elif kind == "override":
        R, f = override_inputs(n)
        e = fly(p, init, acts, wind, objects=fl["objects"], override=(R, f[:k]), auto_reset=auto_reset)
    elif kind == "table":
        e = fly_table(table_sets(p), init, acts, wind=wind, objects=fl["objects"], auto_reset=auto_reset)
    elif kind == "table_reset":
        e = fly_table(table_sets(p), init, acts, wind=wind, reset=reset_source(p, init, n))
    elif kind == "gate":
        rs = reset_source(p, init, n) if row[1] == "reset" else None
        kw = dict(laps=1) if row[1] == "finish" else {}
        e = fly_gates(p, init, acts, gate_rows(row)[1], wind, objects=fl["objects"], auto_reset=auto_reset or rs is not None, reset=rs, **kw)
    elif kind == "reset":
        e = fly(p, init, acts, wind, reset=reset_source(p, init, n))
    else:
        raise KeyError(row)
    e["acts"], e["ns"] = acts, ns
    return e


@functools.lru_cache(maxsize=None)
def host(row, wind=WIND):
    """`fly_row` of the row's 1000 drones over its own 300 steps, computed once; the first n columns are the flight of n drones.
    Read-only."""
    e = fly_row(row, wind=wind)
    for v in e.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return e


def fly_h(p, pos, sh, acts, wind=WIND, seed=5, auto_reset=False):
    """lane_model.run_h one step at a time on the storage (pos [3, ld], sh [11 * ld] uint16, advanced in place): per-step done [k, n]
    and reward [k, n]"""
    k, n = acts.shape[:2]
    done, reward = np.zeros((k, n), bool), np.empty((k, n), np.float32)
    for t in range(k):
        d, r = lane_model.run_h(p, pos, sh, np.ascontiguousarray(acts[t:t + 1]), wind=wind, seed0=seed, n=n, auto_reset=auto_reset, step0=t)
        done[t], reward[t] = d.astype(bool), r
    return done, reward


@functools.lru_cache(maxsize=None)
def host_h(wind=WIND, seed=5):
    """The fp16 row: (pos [3, N], sh [11 * N] uint16 storage words, done, reward) after the flight by lane_model.run_h, from the
    storage `split_half` makes of the starts with rounding seed `seed`; and the storage before the flight"""
    fl = flight("fp16")
    pos, sh = lane_model.split_half(np.ascontiguousarray(fl["init"]), seed=seed)
    pos0, sh0 = pos.copy(), sh.copy()
    done, rew = lane_model.run_h(fl["p"], pos, sh, fl["acts"], wind=wind, seed0=seed, n=N)
    return dict(pos=pos, sh=sh, done=done, reward=rew, pos0=pos0, sh0=sh0)


def compared_lanes(row):
    """the columns of the row whose end the oracle can be asked for: every eighth under the override (its oracle flies one drone at
    a time), the lanes that never ended an episode where lanes reset, all 1000 otherwise"""
    if row[0] == "override":
        return np.arange(0, N, 8)
    if row[0] == "reset" or row == ("gate", "reset"):
        return np.flatnonzero(~host(row, WIND)["done"].any(0) & ~host(row, CALM)["done"].any(0))
    return np.arange(N)


@functools.lru_cache(maxsize=None)
def reference(row, wind=WIND):
    """(lanes, ref [len(lanes), 19]): the float64 oracle's end state of `compared_lanes(row)` flown from the same starts with the
    sticks the row applied, its object list and the wind"""
    fl, lanes = row_flight(row), compared_lanes(row)
    p = fl["p"].replace(objects=fl["objects"]) if fl["objects"] else fl["p"]
    ref = oracle.drone_initial_state(len(lanes), np.asarray(fl["pos"])[lanes], np.asarray(fl["vel"])[lanes], np.asarray(fl["ypr"])[lanes])
    if row[0] == "fp16":
        acts = fl["acts"]
    else:
        acts = host(row, wind)["acts"]
    a64 = np.ascontiguousarray(acts[:, lanes]).astype(np.float64)
    if row[0] == "override":
        R, f = override_inputs(N)
        for j, i in enumerate(lanes):
            st = np.ascontiguousarray(ref[j])
            oracle.drone_run_guided(p, st, a64[:, j], np.broadcast_to(R[i].astype(np.float64), (a64.shape[0], 3, 3)), f[:, i], wind=wind)
            ref[j] = st
    elif row[0] == "table":
        sets = table_sets(fl["p"])
        for k, ps in enumerate(sets):
            sub = np.flatnonzero(lanes % len(sets) == k)
            r = np.ascontiguousarray(ref[sub])
            oracle.drone_run(ps.replace(objects=fl["objects"]) if fl["objects"] else ps, r, np.ascontiguousarray(a64[:, sub]), wind=wind)
            ref[sub] = r
    else:
        oracle.drone_run(p, ref, a64, wind=wind)
    ref.setflags(write=False)
    return lanes, ref


def oracle_error(row, state, n, wind=WIND):
    """parity.soa_vs_oracle of an end state [14, >= n] (the host's or a kernel's) on the row's compared lanes below n, or None when
    there is none below n"""
    lanes, ref = reference(row, wind)
    m = int(np.searchsorted(lanes, n))
    if m == 0:
        return None
    return soa_vs_oracle(np.ascontiguousarray(np.asarray(state)[:, lanes[:m]]), np.ascontiguousarray(ref[:m]), m)
