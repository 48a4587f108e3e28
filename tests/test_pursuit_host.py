"""The pursuit task without a GPU (include/fpv_abi.h "Pursuit task"): the reference's own Target / CircularPath /
generate_targets, captured in tests/golden/g20_targets.npz (tools/gen_pursuit_golden.py), pin the float64 restatement of
tests/pursuit_task.py to 1e-12 and the fp32 host function (fpv_pursuit_eval - the lane function every lane of the kernel runs) to
the rounding of its number format; the rule (advance, pay, capture, respawn, rebase, observe) is held to the restatement over the
seeded scene the GPU test reuses; the respawn draw to oracle/philox.py; the guidance law to fpv_chase_eval, bit for bit; and every
refusal of the C ABI to its message.

Bounds, from the number format (eps = 2^-24, one rounding to nearest): a target coordinate is ONE fmaf(PATH_R, table, centre) of a
table entry rounded once - 2^-23 (|centre| + PATH_R) covers both and nothing accumulates.  With M = |centre|_1 + 2 PATH_R + |p|_1 +
radius (every length of the measurement is below it), w = t - p carries at most 3 roundings of M per component, the norm 3 more of
the range and its input errors times sqrt(3), `- radius` one more: 16 eps M bounds dist and 2 x that a component of R^T w (three
products of |R_ij| <= 1, the entries of R themselves rounded).  The payment adds the error of the previous dist, both times
|progress|, and two roundings of its own size; the relative velocity divides two target coordinates' error by dt.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import pursuit_task as PT
from conftest import REPO, load_golden
from fpyv_amd import _lib, load_params
from fpyv_amd.chase import ChaseGuidance
from fpyv_amd.pursuit import PursuitTask, generate_targets, targets_from_params

ORACLE_TOL = 1e-12
# the largest deviation of the fp32 distance from the reference's over the capture, relative to M (the sum of the magnitudes that
# enter it: |centre|_1 + PATH_R + |point|_1 + radius), is 1.27e-7; asserted with the margin of 8 DESIGN 3.9 uses for
# inputs the capture does not span
FP32_TOL_DISTANCE = 8 * 1.27e-7
PAIRS = [("world", "level"), ("world", "frontarget"), ("drone", "level"), ("drone", "frontarget")]


@pytest.fixture(scope="module")
def golden():
    return load_golden("g20_targets")


@pytest.fixture(scope="module")
def params():
    return load_params(fps=250)


def ident(n):
    q = np.zeros((n, 4), dtype=np.float32)
    q[:, 0] = 1.0
    return q


# ---- H1: against the reference ---------------------------------------------------------------------------------------------------
def test_the_float64_restatement_matches_every_captured_position_and_distance(golden):
    g, worst = golden, 0.0
    for i in range(len(g["radius"])):
        k = int(g["resolution"][i])
        circle = PT.circle64(max(k, 1))
        for u in range(int(g["updates"][i])):
            cs = circle[u % max(k, 1)]
            pos = g["centre"][i] + (g["path_radius"][i] * np.array([cs[0], cs[1], 0.0]) if k else 0.0)
            scale = np.abs(g["centre"][i]).max() + g["path_radius"][i]
            worst = max(worst, np.abs(pos - g["position"][i, u]).max() / scale)
            dist = np.linalg.norm(g["points"][i, u].astype(np.float64) - pos, axis=1) - g["radius"][i]
            worst = max(worst, (np.abs(dist - g["distance"][i, u]) / np.maximum(np.abs(g["distance"][i, u]), 1.0)).max())
    print(f"restatement against the reference: {worst:.2e}")
    assert worst <= ORACLE_TOL


def test_the_fp32_host_function_matches_every_captured_coordinate_and_distance(golden):
    """16 lanes share a target (one per captured point) and advance in step; a reset call with respawn_on_done = 0 measures without
    capturing, so a point inside the sphere does not respawn the target"""
    g, worst = golden, 0.0
    pts = g["points"].shape[2]
    for i in range(len(g["radius"])):
        k = int(g["resolution"][i])
        task = PursuitTask(targets=dict(centre=g["centre"][i], radius=g["radius"][i], path_radius=g["path_radius"][i]),
                           path=dict(resolution=max(k, 1)), respawn_on_done=False)
        rows = task.rows(pts)
        bound = 2.0 ** -23 * (np.abs(g["centre"][i]) + g["path_radius"][i])
        for u in range(int(g["updates"][i])):
            p = g["points"][i, u]
            out = task.evaluate(p, np.zeros((pts, 3)), ident(pts), rows, 0.004, reset=True, advance=k > 0)
            rows = out["rows"]
            err = np.abs(out["position"].astype(np.float64) - g["position"][i, u][:, None])
            assert np.all(err <= bound[:, None]), (i, u, err.max(1), bound)
            m = np.abs(g["centre"][i]).sum() + g["path_radius"][i] + np.abs(p.astype(np.float64)).sum(1) + g["radius"][i]
            worst = max(worst, (np.abs(out["obs"][6].astype(np.float64) - g["distance"][i, u]) / m).max())
            assert np.array_equal(out["rows"][_lib.TGT_PREV_DIST, :pts], out["obs"][6])
    print(f"fp32 distance against the reference, relative to the magnitudes that enter it: {worst:.2e}")
    assert worst <= FP32_TOL_DISTANCE


def test_generate_targets_is_the_references_factory_with_a_seeded_generator(golden):
    g = golden
    section = dict(count=4, center=list(g["section_center"]), std=float(g["section_std"]), size=float(g["section_size"]),
                   variation=float(g["section_variation"]), nu=5, path=dict(radius=25, resolution=5500))
    made = targets_from_params(section, seed=int(g["seed"]))
    assert np.allclose([t.position for t in made], g["generated_centre"], rtol=ORACLE_TOL, atol=0)
    assert np.allclose([t.radius for t in made], g["generated_radius"], rtol=ORACLE_TOL, atol=0)
    assert all(t.path == dict(radius=25, resolution=5500) for t in made)
    again = generate_targets(4, section["center"], section["std"], section["size"], section["variation"], seed=int(g["seed"]))
    assert all(np.array_equal(a.position, b.position) for a, b in zip(made, again)) and again[0].path is None
    rows = PursuitTask(targets=made).rows(4)
    assert np.array_equal(rows[:3, :4].T, np.float32(g["generated_centre"])) and np.all(rows[_lib.TGT_PATH_R, :4] == 25.0)


# ---- H2: the rule ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def flown():
    """the scene through fpv_pursuit_eval and through the restatement: per call (host output, restated output, rows before)"""
    P, V, Q, D, stats = PT.scene()
    task = PT.task(targets=PT.start_targets())
    rows = task.rows(PT.N)
    model = PT.Restated(task, rows, PT.N, PT.DT)
    rng = np.random.default_rng(3)
    calls = []
    for c in range(PT.CALLS):
        step_reward = rng.normal(size=PT.N).astype(np.float32)
        out = task.evaluate(P[c], V[c], Q[c], rows, PT.DT, done=D[c], reward=step_reward, reset=c == 0)
        want = model.call(P[c], V[c], Q[c], done=D[c], reset=c == 0)
        calls.append((out, want, rows, step_reward, model.count_words().copy(), model.spawn_words().copy()))
        rows = out["rows"]
    return task, calls, stats


def test_the_scene_exercises_captures_rebases_double_captures_and_the_exact_threshold():
    stats = PT.scene()[4]
    print(stats)
    assert stats["captures"] >= 20 and stats["rebases"] >= 20 and stats["twice"] >= 1 and stats["exact"] >= 1
    assert stats["near_threshold"] == 0         # no other lane is within fp32 rounding of the threshold: the events are well defined


def test_events_counts_and_path_indices_equal_the_restatement_exactly(flown):
    _, calls, _ = flown
    events = 0
    for c, (out, want, _, _, count, spawns) in enumerate(calls):
        words = out["rows"].view(np.uint32)
        assert np.array_equal(out["event"], want["event"] * want["active"]), c
        assert np.array_equal(words[_lib.TGT_COUNT, :PT.N], count), c
        assert np.array_equal(words[_lib.TGT_SPAWNS, :PT.N], spawns), c
        events += int(out["event"].sum())
    assert events >= 20
    out, want = calls[PT.EXACT_CALL][:2]
    assert out["event"][PT.EXACT] == 1 and out["obs"][6][PT.EXACT] != 0.25           # captured at dist == capture_distance, respawned


def test_rewards_and_observations_equal_the_restatement_at_fp32_rounding(flown):
    task, calls, _ = flown
    for c, (out, want, _, step_reward, _, _) in enumerate(calls):
        a = want["active"]                              # (the reset call leaves the lane outside its mask alone)
        assert np.all(np.abs(out["obs"][6] - want["obs"][6])[a] <= want["tol_dist"][a]), c
        assert np.all(np.abs(out["obs"][:3] - want["obs"][:3])[:, a] <= want["tol_w"][a]), c
        assert np.all(np.abs(out["obs"][3:6] - want["obs"][3:6])[:, a] <= want["tol_v"][a]), c
        assert np.all(np.abs(out["position"] - want["position"])[:, a] <= (2.0 ** -23 * (np.abs(want["position"]) + 8.0))[:, a]), c
        assert not out["obs"][:, ~a].any() and not out["position"][:, ~a].any()
        if c == 0:
            assert not out["paid"].any() and np.array_equal(out["reward"], step_reward)       # a reset call pays nothing
            continue
        assert np.all(np.abs(out["paid"] - want["paid"]) <= want["tol_paid"]), (c, np.abs(out["paid"] - want["paid"]).max())
        # the hand-over: reward = the step's reward + the payment, one fp32 addition; a rebasing lane's cell is not touched
        assert np.array_equal(out["reward"], np.where(want["rebase"], step_reward, step_reward + out["paid"]))


def test_progress_is_never_paid_across_a_respawn_or_a_rebase(flown):
    """a rebasing lane is paid nothing; a lane whose target respawned in the previous call is paid against the distance to its NEW
    target - exactly progress * (that distance - this one), one fp32 subtraction and one product: never the jump"""
    task, calls, _ = flown
    seen = 0
    for c in range(1, len(calls)):
        out, want, rows_before = calls[c][:3]
        rebased = want["rebase"]
        assert not out["paid"][rebased].any() and not out["event"][rebased].any()
        prev_out, prev_want = calls[c - 1][:2]
        assert np.array_equal(rows_before[_lib.TGT_PREV_DIST, :PT.N], prev_out["obs"][6])
        lane = prev_want["respawned"] & ~rebased & ~out["event"].astype(bool)
        paid = np.float32(task.progress) * (prev_out["obs"][6] - out["obs"][6])
        assert np.array_equal(out["paid"][lane], paid[lane]), c
        seen += int(lane.sum())
    assert seen >= 20


def test_without_advance_the_targets_stand_and_a_fresh_target_stays_fresh():
    n = 33
    task = PT.task(targets=PT.start_targets(n))
    P, V, Q, _, _ = PT.scene(n)
    rows = task.rows(n)
    a = task.evaluate(P[0], V[0], Q[0], rows, PT.DT, reset=True, advance=False)
    b = task.evaluate(P[0], V[0], Q[0], a["rows"], PT.DT, done=np.zeros(n), advance=False)
    assert np.array_equal(a["rows"].view(np.uint32)[_lib.TGT_COUNT], b["rows"].view(np.uint32)[_lib.TGT_COUNT])
    quiet = b["event"] == 0
    assert np.array_equal(a["position"][:, quiet], b["position"][:, quiet]) and np.all(a["rows"].view(np.uint32)[_lib.TGT_COUNT, :n] >> 31 == 1)
    c = task.evaluate(P[0], V[0], Q[0], b["rows"], PT.DT, done=np.zeros(n), advance=True)       # the first advance leaves it there
    assert np.array_equal(b["position"][:, quiet], c["position"][:, quiet])
    still = quiet & (c["event"] == 0)
    assert np.all(c["rows"].view(np.uint32)[_lib.TGT_COUNT, :n][still] >> 31 == 0)


# ---- H3: respawn -----------------------------------------------------------------------------------------------------------------
def test_the_respawn_draw_is_philox_of_seed_global_id_and_respawn_index():
    seed, gid, index = 0x0123456789ABCDEF, (7 << 32) | 12345, 41
    raw = PursuitTask(path=dict(resolution=65536), respawn=dict(lo=(0, 0, 0), hi=(2 ** 24,) * 3, radius=(0, 2 ** 24), seed=seed))
    centre, radius, phase = raw.sample(gid, index)
    w0, w1 = PT.words(seed, gid, index)                    # oracle/philox.py, rounds = 7
    assert [int(x) for x in centre] + [int(radius)] == [int(w) >> 8 for w in w0]          # span 2^24, lo 0: the word's top 24 bits
    assert phase == int(w1[0]) >> 16
    # depends on (seed, global id, respawn index) only, and on each of them
    task = PT.task()
    base = task.sample(gid, index)
    again = PT.task(capture_distance=3.0, rewards=dict(progress=0.1, capture=1.0), respawn_on_done=False).sample(gid, index)
    assert np.array_equal(base[0], again[0]) and base[1:] == again[1:]
    for other in (PT.task(respawn=dict(PT.TASK_KW["respawn"], seed=seed)).sample(gid, index), task.sample(gid + 1, index), task.sample(gid, index + 1)):
        assert not np.array_equal(base[0], other[0])
    want = PT.draw64(task.spawn_seed, gid, index, task.spawn_lo, task.spawn_hi, task.radius_lo, task.radius_hi, task.resolution)
    assert np.all(np.abs(base[0] - want[0]) <= 2.0 ** -23 * 6.0) and abs(base[1] - want[1]) <= 2.0 ** -23 and base[2] == want[2]


def test_draws_lie_inside_the_box_ends_included():
    task = PT.task()
    lo, hi = np.float32(task.spawn_lo), np.float32(task.spawn_hi)
    draws = [task.sample(g, k) for g in range(200) for k in range(3)]
    c, r, j = np.array([d[0] for d in draws]), np.array([d[1] for d in draws]), np.array([d[2] for d in draws])
    assert np.all(c >= lo) and np.all(c <= hi) and np.all(r >= np.float32(task.radius_lo)) and np.all(r <= np.float32(task.radius_hi))
    assert j.min() >= 0 and j.max() < task.resolution and len(set(j)) > task.resolution // 2
    assert np.all(c.min(0) < lo + 0.05 * (hi - lo)) and np.all(c.max(0) > hi - 0.05 * (hi - lo))       # it fills the box
    point = PursuitTask(respawn=dict(lo=(1, 2, 3), hi=(1, 2, 3), radius=(0.5, 0.5)))                   # a box that is a point
    assert np.array_equal(point.sample(5, 0)[0], np.float32([1, 2, 3])) and point.sample(5, 0)[1] == 0.5


def test_a_shard_with_a_drone_id_offset_equals_the_columns_of_the_whole_batch():
    n, lo, hi = 256, 100, 164
    P, V, Q, D, _ = PT.scene(n)
    task = PT.task(targets=PT.start_targets())
    whole = task.rows(PT.N)[:, :n].copy()
    shard = whole[:, lo:hi].copy()
    respawned = 0
    for c in range(PT.CALLS):
        kw = dict(dt=PT.DT, reset=c == 0)
        a = task.evaluate(P[c], V[c], Q[c], whole, done=D[c], **kw)
        b = task.evaluate(P[c, lo:hi], V[c, lo:hi], Q[c, lo:hi], shard, done=D[c, lo:hi], drone_id_offset=lo, **kw)
        whole, shard = a["rows"][:, :n], b["rows"][:, :hi - lo]
        for key in ("obs", "position", "event", "paid"):
            assert np.array_equal(a[key][..., lo:hi].view(np.uint8), b[key].view(np.uint8)), (c, key)
        respawned += int(b["event"].sum())
    assert np.array_equal(whole[:, lo:hi].view(np.uint32), shard.view(np.uint32)) and respawned >= 5
    unshifted = task.evaluate(P[0, lo:hi], V[0, lo:hi], Q[0, lo:hi], task.rows(PT.N)[:, lo:hi], PT.DT, reset=True)
    assert not np.array_equal(unshifted["rows"][:3], task.evaluate(P[0, lo:hi], V[0, lo:hi], Q[0, lo:hi], task.rows(PT.N)[:, lo:hi], PT.DT,
                                                                  reset=True, drone_id_offset=lo)["rows"][:3])


# ---- H4: the guidance law against each drone's own target ------------------------------------------------------------------------
@pytest.mark.parametrize("frame,mode", PAIRS)
def test_the_guided_call_equals_fpv_chase_eval_against_each_drones_own_target(params, frame, mode):
    n, calls = 65, 6
    P, V, Q, D, _ = PT.scene(n)
    P = P + np.float32([0.0, 0.0, 1.0])                   # (the scene flies low: some lanes below tof, most above)
    task = PT.task(targets=PT.start_targets(), guide=dict(ref_frame=frame, mode=mode, max_depth=40.0))
    yard = ChaseGuidance(params, ref_frame=frame, mode=mode, max_depth=40.0)
    rows, pid, guided = task.rows(PT.N)[:, :n].copy(), None, 0
    for c in range(calls):
        out = task.evaluate(P[c], V[c], Q[c], rows, PT.DT, done=D[c], reset=c == 0, pid_state=pid, params=params)
        rebased = D[c].astype(bool)
        for i in range(n):
            if c == 0 and not rebased[i]:                 # outside the reset call's mask: not touched
                assert not out["rotation"][i].any() and out["thrust"][i] == 0.0
                continue
            before = np.float32([0, 0, 0, 1]) if (pid is None or rebased[i]) else pid[:, i]
            rot, thrust, pix, vis, st = yard.evaluate(P[c, i], V[c, i], Q[c, i], (out["position"][:, i], out["rows"][_lib.TGT_RADIUS, i]),
                                                      pid_state=before.reshape(4, 1))
            for got, want in ((out["rotation"][i], rot[0]), (out["thrust"][i], thrust[0]), (out["pixel"][i], pix[0]), (out["pid_state"][:, i], st[:, 0])):
                assert np.array_equal(np.asarray(got, dtype=np.float32).view(np.uint32), np.asarray(want, dtype=np.float32).view(np.uint32)), (c, i)
            assert bool(out["visible"][i]) == bool(vis[0])
        guided += int(np.isfinite(out["thrust"]).sum())
        rows, pid = out["rows"][:, :n], out["pid_state"]
    assert guided >= 20, guided


# ---- H5: refusals ----------------------------------------------------------------------------------------------------------------
def test_every_refusal_names_its_reason(params):
    L = _lib.lib()
    n = 4
    task = PT.task(guide=dict())
    rows, zeros = task.rows(n), np.zeros((n, 4), dtype=np.float32)
    obs, reward = np.zeros((7, n), dtype=np.float32), np.zeros(n, dtype=np.float32)
    st, rot, thrust = np.zeros((4, n), dtype=np.float32), np.zeros((n, 9), dtype=np.float32), np.zeros(n, dtype=np.float32)
    keep = []

    def good(guide=False):
        s = task.derive(0.004)
        s.targets, s.targets_ld, s.obs, s.obs_ld = rows.ctypes.data, rows.shape[1], obs.ctypes.data, n
        if guide:
            g = task.chase(params)
            g.pid_state, g.pid_ld, g.rotation, g.thrust = st.ctypes.data, n, rot.ctypes.data, thrust.ctypes.data
            keep.append(g)
            s.guide = C.pointer(g)
        return s

    def refused(s, what, count=n, rew=reward, v=zeros):
        rc = L.fpv_pursuit_eval(C.byref(s) if s is not None else None, count, 0, zeros.ctypes.data, v.ctypes.data if v is not None else None,
                                zeros.ctypes.data, None, rew.ctypes.data if rew is not None else None, 0)
        msg = L.fpv_last_error().decode()
        assert rc < 0 and what in msg, (what, rc, msg)

    assert L.fpv_pursuit_eval(C.byref(good()), n, 0, zeros.ctypes.data, zeros.ctypes.data, zeros.ctypes.data, None, reward.ctypes.data, 0) == 0
    assert L.fpv_pursuit_eval(C.byref(good(True)), n, 0, zeros.ctypes.data, zeros.ctypes.data, zeros.ctypes.data, None, reward.ctypes.data, 0) == 0
    cases = [("struct_size", 0, "struct_size"), ("path_resolution", 0, "path_resolution must be 1..65536"),
             ("path_resolution", 65537, "path_resolution must be 1..65536"), ("dt", 0.0, "dt must be positive"), ("dt", -1.0, "dt must be positive"),
             ("dt", float("nan"), "dt is not finite"), ("capture_distance", -0.5, "capture_distance must not be negative"),
             ("capture_distance", float("inf"), "capture_distance is not finite"), ("progress", float("nan"), "progress is not finite"),
             ("capture", float("inf"), "capture is not finite"), ("radius_lo", -0.1, "radius must not be negative"),
             ("radius_hi", 0.1, "radius range has hi < lo"), ("radius_hi", float("nan"), "radius range is not finite"),
             ("targets", None, "targets is null"), ("circle", None, "circle is null"), ("targets_ld", n - 1, "targets_ld is smaller"),
             ("targets", rows.ctypes.data + 4, "16-byte aligned"),
             ("circle", task.circle.ctypes.data + 4, "circle must be 8-byte aligned"), ("obs", obs.ctypes.data + 2, "4-byte aligned"),
             ("obs_ld", n - 1, "obs_ld is smaller"), ("position", obs.ctypes.data, "position_ld is smaller")]
    for field, value, what in cases:
        s = good()
        setattr(s, field, value)
        refused(s, what)
    s = good(); s.spawn_hi[1] = s.spawn_lo[1] - 1.0; refused(s, "spawn box has hi < lo")
    s = good(); s.spawn_lo[2] = float("nan"); refused(s, "spawn box is not finite")
    refused(good(), "add_to_reward needs", rew=None)
    refused(None, "null argument")
    refused(good(), "n must be positive", count=0)
    refused(good(), "null argument", v=None)
    # everything fpv_chase_guide refuses for the embedded guide
    for field, value, what in (("struct_size", 0, "fpv_chase_t.struct_size"), ("ref_frame", 2, "unknown ref_frame"), ("mode", -1, "unknown mode"),
                               ("mass", -1.0, "mass"), ("max_depth", 0.0, "max_depth"), ("pid_state", None, "pid_state is null"),
                               ("rotation", None, "rotation is null"), ("thrust", None, "thrust is null"), ("pid_ld", 1, "pid_ld"),
                               ("keep_distance", float("nan"), "keep_distance"), ("pixel_out", rot.ctypes.data + 4, "8-byte aligned")):
        s = good(True)
        setattr(keep[-1], field, value)
        refused(s, what)
    s = good(True); keep[-1].target[0] = float("nan"); keep[-1].target_radius = -1.0                  # the shared target is ignored
    assert L.fpv_pursuit_eval(C.byref(s), n, 0, zeros.ctypes.data, zeros.ctypes.data, zeros.ctypes.data, None, reward.ctypes.data, 0) == 0
    # the handle's refusals that need no device; derive and sample
    assert L.fpv_pursuit_step(None, None, C.byref(good()), None) < 0 and b"null handle" in L.fpv_last_error()
    assert L.fpv_pursuit_reset(None, None, C.byref(good()), None, None) < 0 and b"null handle" in L.fpv_last_error()
    assert L.fpv_pursuit_derive(0, zeros.ctypes.data) < 0 and b"path_resolution must be 1..65536" in L.fpv_last_error()
    assert L.fpv_pursuit_derive(4, None) < 0
    out, phase = np.zeros(4, dtype=np.float32), C.c_uint32()
    s = good(); s.spawn_hi[0] = -100.0
    assert L.fpv_pursuit_sample(C.byref(s), 0, 0, out.ctypes.data, C.byref(phase)) < 0 and b"hi < lo" in L.fpv_last_error()
    with pytest.raises(ValueError, match="unknown reward"):
        PursuitTask(rewards=dict(finish=1.0))
    with pytest.raises(ValueError, match="one per drone"):
        PT.task(targets=[1, 2, 3]).rows(5)


def test_the_table_is_the_references_linspace_rounded_once():
    for k in (1, 2, 7, 29, 5500, 65536):
        got, want = PursuitTask(path=dict(resolution=k)).circle, PT.circle64(k)
        assert got.shape == (k, 2) and got.ctypes.data % 8 == 0
        assert np.all(np.abs(got - want) <= 2.0 ** -24)             # |cos|, |sin| <= 1: one rounding
    assert np.array_equal(PursuitTask(path=dict(resolution=4)).circle[0], [1.0, 0.0])


def test_abi_version_struct_size_and_exports():
    L = _lib.lib()
    assert L.fpv_abi_version() == 9 == _lib.FPV_ABI_VERSION
    assert L.fpv_sizeof(0) == C.sizeof(_lib.FpvParams) == 688 and L.fpv_sizeof(1) == C.sizeof(_lib.FpvBuffers) == 200
    assert L.fpv_sizeof(10) == C.sizeof(_lib.FpvPursuit) == 208 and L.fpv_sizeof(9) < 0 and L.fpv_sizeof(11) < 0
    for s in ("fpv_pursuit_derive", "fpv_pursuit_sample", "fpv_pursuit_step", "fpv_pursuit_reset", "fpv_pursuit_eval"):
        assert hasattr(L, s) and s in _lib.EXPORTS


def test_a_library_built_without_the_unit_refuses_by_name(tmp_path):
    """csrc/fpv_hip.hip alone still builds and loads; the three entry points say what is missing (a child process: this one has the
    full library loaded)"""
    import __graft_entry__ as entry
    so = str(tmp_path / "libfpv_alone.so")
    subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + entry.HIPCC_FLAGS + ["-o", so, entry.HIP_SRC], check=True, capture_output=True)
    code = ("import ctypes as C, sys\n"
            "sys.path.insert(0, %r)\n"
            "import torch\n"
            "from fpyv_amd import _lib\n"
            "L = C.CDLL(%r)\n"
            "L.fpv_last_error.restype = C.c_char_p\n"
            "s = _lib.FpvPursuit()\n"
            "assert L.fpv_sizeof(10) == C.sizeof(_lib.FpvPursuit)\n"
            "for rc in (L.fpv_pursuit_eval(C.byref(s), 1, 0, None, None, None, None, None, 0), L.fpv_pursuit_step(None, None, C.byref(s), None),\n"
            "           L.fpv_pursuit_reset(None, None, C.byref(s), None, None)):\n"
            "    assert rc == -1 and b'linked without csrc/fpv_pursuit.hip' in L.fpv_last_error(), L.fpv_last_error()\n"
            "print('refused three times')\n") % (REPO, so)
    r = subprocess.run([os.sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "refused three times" in r.stdout, r.stdout + r.stderr


# ---- the closed loop the GPU test flies, on the CPU first --------------------------------------------------------------------------
def test_the_closed_loop_scene_closes_in_and_captures_on_the_cpu():
    """tests/test_gpu_pursuit.py's scenario (pursuit_task.loop_scene) with fpv_pursuit_eval and the float64 oracle's guided step, for
    the drones that see their target: every one of them captures its target or ends nearer to it than it started, and at least one
    captures - the scene is known to satisfy both before the GPU sees it"""
    from chase_law import quat_of
    from oracle import oracle
    params, n = load_params(fps=PT.LOOP_FPS), PT.LOOP_SEEN
    targets, pos, ypr = PT.loop_scene()
    task = PT.task(targets={k: v[:n] for k, v in targets.items()}, **PT.LOOP_TASK_KW)
    state = oracle.drone_initial_state(n, pos[:n].astype(np.float64), np.zeros(3), ypr[:n].astype(np.float64))

    def pose():
        return state[:, :3], state[:, 3:6], np.array([quat_of(state[i, 6:15].reshape(3, 3)) for i in range(n)])

    out = task.evaluate(*pose(), task.rows(n), params.dt, reset=True, params=params)
    start = out["obs"][6].copy()
    assert np.all(np.abs(start - 8.0) < 1e-3) and out["visible"].all() and start.max() < params.UWB_sensor_max_range
    captured = np.zeros(n, dtype=bool)
    for _ in range(PT.LOOP_STEPS):
        for i in range(n):
            _, _, done = oracle.drone_run_guided(params, state[i], PT.HOVER_STICKS[None], out["rotation"][i][None], np.array([out["thrust"][i]]))
            assert not done.any()
        out = task.evaluate(*pose(), out["rows"], params.dt, done=np.zeros(n), params=params, pid_state=out["pid_state"])
        captured |= out["event"].astype(bool)
    print(f"{int(captured.sum())} of {n} captured; the others end at {np.sort(out['obs'][6][~captured]).round(2)} m")
    assert captured.sum() >= 1 and np.all(captured | (out["obs"][6] < start))
