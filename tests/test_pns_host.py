"""Point and shoot on the host, no GPU: the float64 restatement of the law (tests/pns_law.py) against the reference captures
g21_pns_calls / g21_pns_loop (tools/gen_pns_golden.py) at the oracle tolerance - the limited calls included, where the restatement
takes the closed form and the capture holds the reference loop's result; the library's fp32 lane function (fpv_pns_eval, the function
the kernel runs) against the same captures call by call; the cases the build defines where the reference gives NaN or does not
return; and the C ABI - sizes, every refusal by name, a library built without the unit."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from chase_law import quat_of
from conftest import REPO, load_golden
from pns_law import PnsLaw

from fpyv_amd import _lib, load_params
from fpyv_amd.pns import PointAndShoot

ORACLE_TOL = 1e-12
# fpv_pns_eval (fp32) against the reference captures (float64), inputs narrowed to fp32.  Measured over both g21 files:
# 4.1e-6 on a matrix entry, 2.8e-7 relative on the force, 2.4e-7 on the throttle (a value in [-1, 1]); the bounds are those with the
# margin of 8 that 3.9 takes for inputs the captures do not span
FP32_TOL_MATRIX = 8 * 4.1e-6
FP32_TOL_FORCE = 8 * 2.8e-7
FP32_TOL_THROTTLE = 8 * 2.4e-7
# the PID rows after a call, from the number format.  The error row is pixel.y + a3 H/2 - position.y: a pixel coordinate of the
# captures is below 1024 in magnitude (asserted), where an fp32 value is within 2^-14 = 6.1e-5 of the float64 one; the recorded pixel
# is narrowed once and the sum with the offset is rounded once: two such roundings.  The integral row moves by dt times that plus four
# roundings of a value below 16 (asserted; 4.8e-7 each: the recorded row narrowed, the product, the fma, the clip's operand).  The
# derivative row is the difference of two such errors divided by dt and scaled by the filter's rate, plus the roundings of a value
# below 1.  prev_pixel is the pixel itself: the error row's bound; the pixel velocity is the difference of two of them over dt.
FP32_TOL_PIXEL = 2 * 2.0 ** -14
PAIRS = [("world", "level"), ("world", "frontarget"), ("drone", "level"), ("drone", "frontarget")]


@pytest.fixture(scope="module")
def calls():
    return load_golden("g21_pns_calls")


@pytest.fixture(scope="module")
def loop():
    return load_golden("g21_pns_loop")


@pytest.fixture(scope="module")
def params():
    return load_params(fps=250)


def fresh():
    return np.array([0.0, 0.0, 0.0, 1.0])


NONE = np.full(2, np.nan)


def rel(a, b):
    """|a - b| relative to the quantity's magnitude"""
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(1.0, float(np.max(np.abs(b)))))


def test_the_captures_are_what_the_issue_asks_for(calls, loop):
    assert [str(x) for x in calls["pairs"]] == ["/".join(p) for p in PAIRS]
    assert calls["p"].shape == (4, 64, 3) and loop["p"].shape == (300, 4, 3)
    for k in ("p", "v", "ypr", "pixel", "action"):
        assert np.array_equal(calls[k], calls[k].astype(np.float32).astype(np.float64)), k
    speed = np.linalg.norm(calls["v"], axis=-1)
    assert speed.min() >= 0.1
    sinking = (calls["p"][..., 2] < calls["tof_effective_distance"]) & (calls["v"][..., 2] < 0)
    assert sinking.mean() >= 0.25                                       # a quarter below tof with v.z < 0
    assert calls["entered"].mean() == 0.25                              # a quarter with the limit binding ...
    assert np.all((speed[calls["entered"] == 1] >= 12.0) & (speed[calls["entered"] == 1] <= 25.0))     # ... drawn at 12..25 m/s
    assert np.abs(calls["action"]).max() <= 1.0 and np.all(np.ptp(calls["action"], axis=(0, 1)) > 1.9)
    fmax = float(calls["max_throttle_in_force"])
    hit = calls["entered"] == 1
    assert np.all(np.abs(calls["force"][hit] - fmax) <= 1e-12 * fmax) and np.all(calls["force"][~hit] <= fmax)
    # the sine between F and the second operand of the first cross product
    g = np.array([0.0, 0.0, -9.81 * float(calls["mass"])])
    law = PnsLaw.from_golden(calls)
    for k, (frame, mode) in enumerate(PAIRS):
        for i in range(64):
            R, F = calls["R"][k, i], calls["rot"][k, i][:, 2]
            if mode == "level":
                b = R @ g if frame == "drone" else g
            else:
                pix = calls["pixel"][k, i] + calls["action"][k, i, 2:] * np.array([law.w / 2, law.h / 2])
                b = R @ (law.rr @ np.array([(pix[0] - law.w / 2) / law.f, (pix[1] - law.h / 2) / law.f, 1.0]))
            assert np.linalg.norm(np.cross(F, b)) / np.linalg.norm(b) >= 0.05 * (1 - 1e-9)
    assert 0 < loop["seen"].sum() < loop["seen"].size                # both branches of simulator.py:104 are flown
    assert np.all(np.any(loop["commands"][:, 1:] != 0.0, axis=1))      # one fixed non-zero command per drone
    for g21 in (calls, loop):                                         # what the PID bounds above assume
        assert np.nanmax(np.abs(g21["pid_after"][..., 0])) < 16.0


def test_the_packaged_parameters_are_the_captures(calls, params):
    law, ref = PnsLaw.from_params(params), PnsLaw.from_golden(calls)
    for k in ("f", "w", "h", "vdrag", "vlift", "tof", "kP", "kI", "kD", "dt", "iclip", "lo", "hi", "drate", "max_depth", "fmax"):
        assert abs(getattr(law, k) - getattr(ref, k)) <= 1e-12 * max(1.0, abs(getattr(ref, k))), k
    # DroneParams.thrust2throttle_poly against the coefficients of the reference's own model_xy(thrust, throttle)
    assert np.all(np.abs(params.thrust2throttle_poly - calls["thrust2throttle_poly"]) <= 1e-9 * np.abs(calls["thrust2throttle_poly"]))
    for f in (1.0, 7.0, 40.0, 81.0, 200.0):
        assert params.thrust2throttle(f) == pytest.approx(ref.throttle(f), abs=1e-12)
    assert abs(params.thrust2throttle(100.0)) <= 1.0
    assert PointAndShoot(params).ref_frame == "world" and PointAndShoot(params).mode == "level"


def test_float64_restatement_matches_every_single_call_of_the_reference(calls):
    law = PnsLaw.from_golden(calls)
    worst, limited = 0.0, 0
    for k, (frame, mode) in enumerate(PAIRS):
        for i in range(64):
            o = law(calls["p"][k, i], calls["v"][k, i], calls["R"][k, i], calls["action"][k, i], fresh(), NONE, pixel=calls["pixel"][k, i],
                    frame=frame, mode=mode)
            assert o["guided"] and o["limited"] == int(calls["entered"][k, i])
            limited += o["limited"]
            worst = max(worst, rel(o["rot"], calls["rot"][k, i]), rel(o["thrust"], calls["force"][k, i]), rel(o["pid"], calls["pid_after"][k, i]),
                        rel(o["throttle"], calls["throttle"][k, i]), rel(o["prev"], calls["prev_pixel"][k, i]),
                        rel(o["velocity"], calls["pixel_velocity"][k, i]))
            assert o["pid"][2] == pytest.approx(calls["pid_error"][k, i], rel=ORACLE_TOL, abs=ORACLE_TOL)
            assert o["pid"][1] == pytest.approx(calls["pid_derivative"][k, i], rel=ORACLE_TOL, abs=ORACLE_TOL)
    print(f"restatement vs single calls: {worst:.2e} ({limited} limited calls)")
    assert limited == 64 and worst <= ORACLE_TOL


def test_float64_restatement_matches_every_step_of_the_reference_loop(loop):
    law = PnsLaw.from_golden(loop)
    worst = 0.0
    for t in range(loop["p"].shape[0]):
        for k, (frame, mode) in enumerate(PAIRS):
            pixel, depth, seen = law.project(loop["p"][t, k], loop["R"][t, k], loop["target"][t, k])
            assert seen == bool(loop["seen"][t, k])
            o = law(loop["p"][t, k], loop["v"][t, k], loop["R"][t, k], loop["commands"][k], loop["pid_before"][t, k],
                    loop["prev_pixel_before"][t, k], target=loop["target"][t, k], frame=frame, mode=mode)
            assert o["guided"] == seen
            worst = max(worst, rel(o["pid"], loop["pid_after"][t, k]))
            assert np.array_equal(np.isnan(o["prev"]), np.isnan(loop["prev_pixel_after"][t, k]))
            if seen:
                worst = max(worst, rel(pixel, loop["pixel"][t, k]), rel(o["rot"], loop["rot"][t, k]), rel(o["thrust"], loop["force"][t, k]),
                            rel(o["throttle"], loop["throttle"][t, k]), rel(o["prev"], loop["prev_pixel_after"][t, k]),
                            rel(o["velocity"], loop["pixel_velocity"][t, k]))
            else:
                assert np.isnan(o["thrust"]) and np.array_equal(o["rot"], np.eye(3)) and np.isnan(loop["force"][t, k])
    print(f"restatement vs loop: {worst:.2e}")
    assert worst <= ORACLE_TOL


def quats(R):
    return np.array([quat_of(r) for r in R.reshape(-1, 3, 3)])


def test_fp32_host_function_matches_the_reference_captures_call_by_call(calls, loop, params):
    em = ef = et = ev = epp = 0.0
    ep = np.zeros(4)
    rate = params.force_multiplier_pid["derivative_transition_rate"]
    tol_rows = np.array([params.dt * FP32_TOL_PIXEL + 2e-6, 2 * FP32_TOL_PIXEL / params.dt * rate + 1e-6, FP32_TOL_PIXEL, 0.0])
    tol_velocity = 2 * FP32_TOL_PIXEL / params.dt
    for k, (frame, mode) in enumerate(PAIRS):
        G = PointAndShoot(params, ref_frame=frame, mode=mode)
        for i in range(64):
            o = G.evaluate(calls["p"][k, i:i + 1], calls["v"][k, i:i + 1], quats(calls["R"][k, i]), pixel=calls["pixel"][k, i:i + 1],
                           action=calls["action"][k, i])
            assert o["visible"][0] and o["limited"][0] == int(calls["entered"][k, i])
            assert np.abs(calls["pixel"][k, i]).max() < 1024 and np.abs(o["prev_pixel"]).max() < 1024
            em = max(em, float(np.abs(o["rotation"][0] - calls["rot"][k, i]).max()))
            ef = max(ef, abs(float(o["thrust"][0]) - calls["force"][k, i]) / calls["force"][k, i])
            et = max(et, abs(float(o["throttle"][0]) - calls["throttle"][k, i]))
            ep = np.maximum(ep, np.abs(o["pid_state"][:, 0] - calls["pid_after"][k, i]))
            epp = max(epp, float(np.abs(o["prev_pixel"][:, 0] - calls["prev_pixel"][k, i]).max()))
            assert np.array_equal(o["pixel_velocity"][0], [0.0, 0.0])
        # the loop: every step is fed the reference's recorded inputs and state, nothing accumulates
        for t in range(loop["p"].shape[0]):
            seen = bool(loop["seen"][t, k])
            o = G.evaluate(loop["p"][t, k:k + 1], loop["v"][t, k:k + 1], quats(loop["R"][t, k]), action=loop["commands"][k],
                           pixel=loop["pixel"][t, k:k + 1] if seen else np.full((1, 2), np.nan), pid_state=loop["pid_before"][t, k].reshape(4, 1),
                           prev_pixel=loop["prev_pixel_before"][t, k].reshape(2, 1))
            assert bool(o["visible"][0]) == seen
            ep = np.maximum(ep, np.abs(o["pid_state"][:, 0] - loop["pid_after"][t, k]))
            if seen:
                em = max(em, float(np.abs(o["rotation"][0] - loop["rot"][t, k]).max()))
                ef = max(ef, abs(float(o["thrust"][0]) - loop["force"][t, k]) / loop["force"][t, k])
                et = max(et, abs(float(o["throttle"][0]) - loop["throttle"][t, k]))
                epp = max(epp, float(np.abs(o["prev_pixel"][:, 0] - loop["prev_pixel_after"][t, k]).max()))
                ev = max(ev, float(np.abs(o["pixel_velocity"][0] - loop["pixel_velocity"][t, k]).max()))
            else:
                assert np.isnan(o["thrust"][0]) and np.array_equal(o["rotation"][0], np.eye(3, dtype=np.float32))
                assert np.array_equal(o["prev_pixel"][:, 0], loop["prev_pixel_before"][t, k].astype(np.float32), equal_nan=True)
    print(f"fpv_pns_eval vs captures: matrix {em:.2e}, force {ef:.2e} relative, throttle {et:.2e}, PID rows {ep} (bounds {tol_rows}), "
          f"prev_pixel {epp:.2e} (bound {FP32_TOL_PIXEL:.2e}), pixel velocity {ev:.2e} (bound {tol_velocity:.2e})")
    assert em <= 1e-5 and ef <= 1e-5                                  # a measured error above 1e-5 would be a finding
    assert em <= FP32_TOL_MATRIX and ef <= FP32_TOL_FORCE and et <= FP32_TOL_THROTTLE
    assert np.all(ep <= tol_rows) and epp <= FP32_TOL_PIXEL and ev <= tol_velocity


def test_found_pixel_with_a_shared_target_and_with_target_rows_is_the_given_pixel(params):
    """pixel == NULL: the projection of one shared centre and of per-drone rows equals a call given that pixel"""
    law, G = PnsLaw.from_params(params), PointAndShoot(params)
    rng = np.random.default_rng(2)
    n = 40
    p = rng.uniform([-3, -3, 1], [3, 3, 6], (n, 3)).astype(np.float32)
    v = rng.uniform(-3, 3, (n, 3)).astype(np.float32)
    q = np.tile(np.array([1.0, 0, 0, 0], dtype=np.float32), (n, 1))
    c = p + rng.uniform([4, -3, 1], [9, 3, 6], (n, 3)).astype(np.float32)
    c[::5] = p[::5] - np.array([5.0, 0, 0], dtype=np.float32)                  # behind: not seen
    a = rng.uniform(-0.3, 0.3, (n, 4)).astype(np.float32)
    rows = G.evaluate(p, v, q, action=a, target=np.ascontiguousarray(c.T))
    assert 0 < rows["visible"].sum() < n and not rows["visible"][::5].any()
    pix = np.array([law.project(p[i].astype(np.float64), np.eye(3), c[i].astype(np.float64))[0] for i in range(n)])
    given = G.evaluate(p, v, q, action=a, pixel=np.where(rows["visible"][:, None], pix, np.nan))
    s = rows["visible"]
    assert np.array_equal(given["visible"], s) and np.all(np.isnan(rows["thrust"][~s]))
    assert np.abs(rows["rotation"][s] - given["rotation"][s]).max() <= FP32_TOL_MATRIX
    assert np.abs(rows["thrust"][s] / given["thrust"][s] - 1).max() <= 1e-4             # (the PID's gain on a pixel's fp32 rounding)
    one = G.evaluate(p, v, q, action=a, target=c[1])
    same = G.evaluate(p, v, q, action=a, target=np.ascontiguousarray(np.tile(c[1], (n, 1)).T))
    for k in ("rotation", "thrust", "throttle", "pixel_velocity", "limited", "visible", "pid_state", "prev_pixel"):
        assert np.array_equal(one[k], same[k], equal_nan=True), k


# ---- defined where the reference gives NaN or does not return -----------------------------------------------------------------
def orthonormal(rot, thrust, F=None):
    assert np.all(np.isfinite(rot)) and np.isfinite(thrust)
    assert np.abs(rot.T.astype(np.float64) @ rot.astype(np.float64) - np.eye(3)).max() <= 1e-6
    if F is not None:
        assert np.abs(rot[:, 2] - F / np.linalg.norm(F)).max() <= 1e-6


CENTRE = [[320.0, 240.0]]
LEVEL = [[1.0, 0.0, 0.0, 0.0]]


@pytest.mark.parametrize("frame,mode", PAIRS)
def test_zero_velocity_gives_zero_drag_and_a_finite_frame(params, frame, mode):
    law = PnsLaw.from_params(params)
    o = PointAndShoot(params, ref_frame=frame, mode=mode).evaluate([[0, 0, 5]], [[0, 0, 0]], LEVEL, pixel=[[300.0, 200.0]], action=[0.1, 0.2, 0.1, -0.1])
    want = law([0, 0, 5], np.zeros(3), np.eye(3), [0.1, 0.2, 0.1, -0.1], fresh(), NONE, pixel=[300.0, 200.0], frame=frame, mode=mode)
    assert o["visible"][0] and want["guided"]
    orthonormal(o["rotation"][0], o["thrust"][0], want["rot"][:, 2])
    assert np.abs(o["rotation"][0] - want["rot"]).max() <= FP32_TOL_MATRIX and abs(o["thrust"][0] - want["thrust"]) <= FP32_TOL_FORCE * want["thrust"]


def test_force_vertical_in_level_takes_the_fallback_axis(params):
    """level: a pixel whose direction is straight up and no velocity: F = m d - g is vertical, F x g = 0"""
    law = PnsLaw.from_params(params)
    up = law.rr.T @ np.array([0.0, 0.0, 1.0])
    pixel = np.array([[law.f * up[0] / up[2] + law.w / 2, law.f * up[1] / up[2] + law.h / 2]])
    o = PointAndShoot(params, ref_frame="world", mode="level").evaluate([[0, 0, 5]], [[0, 0, 0]], LEVEL, pixel=pixel)
    assert o["visible"][0]
    orthonormal(o["rotation"][0], o["thrust"][0], np.array([0.0, 0.0, 1.0]))
    assert np.abs(o["rotation"][0][:, 1] - [0.0, 1.0, 0.0]).max() <= 1e-6          # y = F x (1, 0, 0) normalised, F along +z


def eval_struct(s, p, v, q, st=None, prev=None, pixel=None, action=None):
    """fpv_pns_eval on a caller-edited struct, one drone: (rc, rotation, thrust, limited, st, prev)"""
    st = np.array([[0.0], [0.0], [0.0], [1.0]], dtype=np.float32) if st is None else st
    prev = np.full((2, 1), np.nan, dtype=np.float32) if prev is None else prev
    rot, thrust, lim = np.zeros((1, 9), dtype=np.float32), np.zeros(1, dtype=np.float32), np.zeros(1, dtype=np.uint8)
    pix = np.zeros(4, dtype=np.float32)
    pix = pix[(-pix.ctypes.data % 8) // 4:][:2]
    pix[:] = CENTRE[0] if pixel is None else pixel
    s.pixel, s.pid_state, s.pid_ld, s.prev_pixel, s.prev_pixel_ld = pix.ctypes.data, st.ctypes.data, 1, prev.ctypes.data, 1
    s.rotation, s.thrust, s.limited = rot.ctypes.data, thrust.ctypes.data, lim.ctypes.data
    arr = [np.asarray(x, dtype=np.float32) for x in (p, v, q)]
    rc = _lib.lib().fpv_pns_eval(C.byref(s), 1, *(a.ctypes.data for a in arr))
    return rc, rot.reshape(3, 3), thrust[0], lim[0], st, prev


def test_zero_force_gives_the_identity_and_zero_thrust(params):
    """F = 0 (|F|^2 below 2^-96, fpv_chase.h 4.): a multiplier pinned to 0 by min_output = max_output = 0, no velocity, above tof
    and a mass of 1e-30 kg: F = -g = (0, 0, 9.81e-30)"""
    s = PointAndShoot(params).derive()
    s.mass, s.pid.min_output, s.pid.max_output = 1e-30, 0.0, 0.0
    rc, rot, thrust, lim, st, _ = eval_struct(s, [[0, 0, 5]], [[0, 0, 0]], LEVEL)
    assert rc == 0 and thrust == 0.0 and lim == 0 and np.array_equal(rot, np.eye(3, dtype=np.float32))
    assert st[3, 0] == 0.0                                              # guided: the PID advanced


def test_limit_out_of_reach_flies_the_limit_along_the_force_of_the_smallest_multiplier(params):
    """40 m/s straight away from the target: the virtual drag alone is 800 N against Fmax = 81 N; the reference's loop does not return"""
    law = PnsLaw.from_params(params)
    for frame, mode in PAIRS:
        o = PointAndShoot(params, ref_frame=frame, mode=mode).evaluate([[0, 0, 5]], [[-40, 3, 1]], LEVEL, pixel=CENTRE, action=[0, 0.2, 0, 0])
        want = law([0, 0, 5], [-40, 3, 1], np.eye(3), [0, 0.2, 0, 0], fresh(), NONE, pixel=CENTRE[0], frame=frame, mode=mode)
        assert o["limited"][0] == 2 == want["limited"] and o["thrust"][0] == np.float32(params.max_throttle_in_force)
        orthonormal(o["rotation"][0], o["thrust"][0], want["rot"][:, 2])
        assert np.abs(o["rotation"][0] - want["rot"]).max() <= FP32_TOL_MATRIX
        assert o["throttle"][0] == pytest.approx(law.throttle(law.fmax), abs=FP32_TOL_THROTTLE)
    # ... and a negative discriminant: |B| > Fmax with B across d
    o = PointAndShoot(params).evaluate([[0, 0, 5]], [[0, 40, 0]], LEVEL, pixel=CENTRE)
    want = law([0, 0, 5], [0, 40, 0], np.eye(3), None, fresh(), NONE, pixel=CENTRE[0])
    assert o["limited"][0] == 2 == want["limited"] and np.abs(o["rotation"][0] - want["rot"]).max() <= FP32_TOL_MATRIX


def test_a_limited_lane_flies_exactly_the_limit(params):
    law = PnsLaw.from_params(params)
    o = PointAndShoot(params).evaluate([[0, 0, 5]], [[8, 21.25, 0]], LEVEL, pixel=[[320.0, 470.0]], action=[0, -0.9, 0, 0])
    want = law([0, 0, 5], [8, 21.25, 0], np.eye(3), [0, -0.9, 0, 0], fresh(), NONE, pixel=[320.0, 470.0])
    assert want["limited"] == 1 == o["limited"][0] and o["thrust"][0] == np.float32(params.max_throttle_in_force)
    assert np.abs(o["rotation"][0] - want["rot"]).max() <= FP32_TOL_MATRIX


@pytest.mark.parametrize("bad", [[np.nan, 0, 0, 0], [0, np.inf, 0, 0], [0, 0, -np.inf, 0], [0, 0, 0, np.nan]])
def test_an_action_that_is_not_finite_leaves_the_drone_unguided_and_its_rows_untouched(params, bad):
    st, prev = np.array([[0.3], [-0.2], [1.5], [0.0]], dtype=np.float32), np.array([[300.0], [200.0]], dtype=np.float32)
    o = PointAndShoot(params).evaluate([[0, 0, 5]], [[1, 0, 0]], LEVEL, pixel=CENTRE, action=bad, pid_state=st, prev_pixel=prev)
    assert not o["visible"][0] and np.isnan(o["thrust"][0]) and np.isnan(o["throttle"][0]) and np.all(np.isnan(o["pixel_velocity"]))
    assert o["limited"][0] == 0 and np.array_equal(o["rotation"][0], np.eye(3, dtype=np.float32))
    assert np.array_equal(o["pid_state"], st) and np.array_equal(o["prev_pixel"], prev)
    ok = PointAndShoot(params).evaluate([[0, 0, 5]], [[1, 0, 0]], LEVEL, pixel=CENTRE, action=[0, 0, 0, 0], pid_state=st, prev_pixel=prev)
    assert ok["visible"][0] and np.isfinite(ok["thrust"][0]) and not np.array_equal(ok["pid_state"], st)


def test_a_nan_pixel_is_an_unseen_target_and_a_null_action_is_zeros(params):
    G = PointAndShoot(params)
    pixel = np.array([[320.0, 240.0], [np.nan, 100.0], [100.0, np.nan]])
    o = G.evaluate(np.zeros((3, 3)) + [0, 0, 5], np.ones((3, 3)), np.tile(LEVEL[0], (3, 1)), pixel=pixel)
    assert list(o["visible"]) == [True, False, False] and np.isfinite(o["thrust"][0]) and np.all(np.isnan(o["thrust"][1:]))
    assert list(o["pid_state"][3]) == [0.0, 1.0, 1.0] and np.all(np.isnan(o["prev_pixel"][:, 1:]))
    z = G.evaluate(np.zeros((3, 3)) + [0, 0, 5], np.ones((3, 3)), np.tile(LEVEL[0], (3, 1)), pixel=pixel, action=[0, 0, 0, 0])
    for k in o:
        assert np.array_equal(o[k], z[k], equal_nan=True), k


def test_the_first_call_has_no_pixel_velocity_and_the_second_has(params):
    G = PointAndShoot(params)
    a = [0.0, 0.1, 0.25, -0.5]
    one = G.evaluate([[0, 0, 5]], [[1, 0, 0]], LEVEL, pixel=[[300.0, 200.0]], action=a)
    assert np.array_equal(one["pixel_velocity"], [[0.0, 0.0]])
    assert np.array_equal(one["prev_pixel"][:, 0], np.float32([300.0 + 0.25 * 320, 200.0 - 0.5 * 240]))       # the law's pixel: offset added
    two = G.evaluate([[0, 0, 5]], [[1, 0, 0]], LEVEL, pixel=[[302.0, 199.0]], action=a, pid_state=one["pid_state"], prev_pixel=one["prev_pixel"])
    assert np.allclose(two["pixel_velocity"], [[2.0 * 250, -1.0 * 250]], rtol=1e-6)
    assert np.array_equal(two["prev_pixel"][:, 0], np.float32([382.0, 79.0])) and two["pid_state"][3, 0] == 0.0
    assert two["pid_state"][1, 0] != 0.0                                  # the derivative row moved: not the first call


def test_restart_resets_the_pid_and_prev_pixel_before_the_call(params):
    G = PointAndShoot(params)
    st, prev = np.array([[0.3, 0.3, 0.3], [-0.2, -0.2, -0.2], [1.5, 1.5, 1.5], [0.0, 0.0, 0.0]], dtype=np.float32), np.full((2, 3), 250.0, dtype=np.float32)
    p, v, q = np.zeros((3, 3)) + [0, 0, 5], np.ones((3, 3)), np.tile(LEVEL[0], (3, 1))
    pixel = np.array([[300.0, 200.0], [300.0, 200.0], [np.nan, np.nan]])
    o = G.evaluate(p, v, q, pixel=pixel, pid_state=st, prev_pixel=prev, restart=[1, 0, 1])
    new = G.evaluate(p, v, q, pixel=pixel)
    for k in o:                                                         # lane 0: a fresh drone's call
        assert np.array_equal(o[k][..., 0] if k in ("pid_state", "prev_pixel") else o[k][0], new[k][..., 0] if k in ("pid_state", "prev_pixel") else new[k][0]), k
    assert np.any(o["pixel_velocity"][1] != 0.0) and o["pid_state"][0, 1] != o["pid_state"][0, 0]              # lane 1 went on
    # lane 2: restarted and then not guided - the reset rows are stored all the same
    assert np.isnan(o["thrust"][2]) and list(o["pid_state"][:, 2]) == [0.0, 0.0, 0.0, 1.0] and np.all(np.isnan(o["prev_pixel"][:, 2]))


# ---- the C ABI -------------------------------------------------------------------------------------------------------------
def test_struct_size_exports_and_the_build_list():
    L = _lib.lib()
    assert L.fpv_abi_version() == 9 == _lib.FPV_ABI_VERSION
    assert L.fpv_sizeof(0) == C.sizeof(_lib.FpvParams) == 688 and L.fpv_sizeof(1) == C.sizeof(_lib.FpvBuffers) == 200
    assert L.fpv_sizeof(12) == C.sizeof(_lib.FpvPns) and L.fpv_sizeof(11) < 0 and b"12 = fpv_pns_t" in L.fpv_last_error()
    import __graft_entry__ as entry
    assert entry.HIP_SRCS_PNS == entry.HIP_SRCS_LINK + [os.path.join(REPO, "fpyv_amd", "csrc", "fpv_pns.hip")]
    assert all(hasattr(L, s) for s in ("fpv_pns_derive", "fpv_pns_guide", "fpv_pns_eval")) and "fpv_pns_guide" in _lib.EXPORTS


def test_every_refusal_names_its_reason(params):
    L = _lib.lib()
    G = PointAndShoot(params)
    n = 2
    st, prev = np.zeros((4, n), dtype=np.float32), np.zeros((2, n), dtype=np.float32)
    rot, thrust, centre = np.zeros((n, 9), dtype=np.float32), np.zeros(n, dtype=np.float32), np.array([1, 2, 3], dtype=np.float32)
    rows = np.zeros((3, n), dtype=np.float32)
    zeros = np.zeros((n, 4), dtype=np.float32)

    def good():
        s = G.derive()
        s.pid_state, s.pid_ld, s.prev_pixel, s.prev_pixel_ld = st.ctypes.data, n, prev.ctypes.data, n
        s.rotation, s.thrust, s.target = rot.ctypes.data, thrust.ctypes.data, centre.ctypes.data
        return s

    def refused(s, what, count=n, v=zeros):
        rc = L.fpv_pns_eval(C.byref(s) if s is not None else None, count, zeros.ctypes.data, v.ctypes.data if v is not None else None, zeros.ctypes.data)
        msg = L.fpv_last_error().decode()
        assert rc < 0 and what in msg, (rc, msg, what)

    assert L.fpv_pns_eval(C.byref(good()), n, zeros.ctypes.data, zeros.ctypes.data, zeros.ctypes.data) == 0
    a16 = rot.ctypes.data + (-rot.ctypes.data % 16)
    cases = [("struct_size", 0, "fpv_pns_t.struct_size"), ("width", 0, "width and height"), ("height", 20000, "width and height"),
             ("ref_frame", 2, "unknown ref_frame"), ("mode", -1, "unknown mode"), ("focal_length", float("nan"), "focal_length"),
             ("max_depth", 0.0, "max_depth"), ("mass", -1.0, "mass"), ("virtual_drag_coefficient", float("nan"), "virtual_drag_coefficient"),
             ("virtual_lift_coefficient", float("inf"), "virtual_lift_coefficient"), ("tof_effective_distance", float("nan"), "tof_effective_distance"),
             ("max_throttle_in_force", 0.0, "max_throttle_in_force"), ("max_throttle_in_force", float("nan"), "max_throttle_in_force"),
             ("pid_state", None, "pid_state is null"), ("prev_pixel", None, "prev_pixel is null"), ("rotation", None, "rotation is null"),
             ("thrust", None, "thrust is null"), ("pid_ld", 1, "pid_ld"), ("prev_pixel_ld", 1, "prev_pixel_ld"),
             ("rotation", rot.ctypes.data + 2, "4-byte aligned"), ("prev_pixel", prev.ctypes.data + 2, "4-byte aligned"),
             ("pixel", a16 + 4, "8-byte aligned"), ("pixel_velocity", a16 + 4, "8-byte aligned"), ("action", a16 + 8, "16-byte aligned"),
             ("target_rows", rows.ctypes.data, "both a shared target and target_rows"), ("target", None, "neither target nor target_rows")]
    for field, value, what in cases:
        s = good()
        setattr(s, field, value)
        refused(s, what)
    s = good(); s.target = None; s.target_rows, s.target_ld = rows.ctypes.data, 1; refused(s, "target_ld")
    s = good(); s.relative_rotation[4] = float("nan"); refused(s, "relative_rotation")
    s = good(); s.thrust2throttle_poly[2] = float("inf"); refused(s, "thrust2throttle_poly")
    s = good(); centre[1] = np.inf; refused(s, "target's centre"); centre[1] = 2.0
    s = good(); s.pid.struct_size = 8; refused(s, "fpv_pns_t.pid.struct_size")
    s = good(); s.pid.dt = 0.0; refused(s, "dt must be positive")
    s = good(); s.pid.kI = float("nan"); refused(s, "PID constant")
    s = good(); s.pid.min_output = 2.0; s.pid.max_output = 1.0; refused(s, "min_output <= max_output")
    refused(None, "null argument")
    refused(good(), "n must be positive", count=0)
    refused(good(), "null argument", v=None)
    assert L.fpv_pns_guide(None, None, C.byref(good()), None) < 0 and b"null handle" in L.fpv_last_error()
    # derive: the numbers of fpv_chase_derive, and its refusals
    cam, out, ref = _lib.FpvCamera(), _lib.FpvPns(), _lib.FpvChase()
    cam.pitch_deg, cam.fov_deg, cam.width, cam.height = 35.0, 120.0, 640, 480
    assert L.fpv_pns_derive(C.byref(cam), C.byref(out)) == 0 and L.fpv_chase_derive(C.byref(cam), C.byref(ref)) == 0
    assert out.focal_length == ref.focal_length and list(out.relative_rotation) == list(ref.relative_rotation) and (out.width, out.height) == (640, 480)
    cam.fov_deg = 180.0
    assert L.fpv_pns_derive(C.byref(cam), C.byref(out)) < 0 and b"fov" in L.fpv_last_error()
    assert L.fpv_pns_derive(None, C.byref(out)) < 0
    with pytest.raises(ValueError, match="Unknown reference frame"):
        PointAndShoot(params, ref_frame="camera")
    with pytest.raises(ValueError, match="Unknown mode"):
        PointAndShoot(params, mode="sideways")


def test_a_library_built_without_the_unit_refuses_by_name(tmp_path):
    """csrc/fpv_hip.hip alone still builds and loads; fpv_pns_guide and fpv_pns_eval say what is missing (a child process: this one
    has the full library loaded)"""
    import __graft_entry__ as entry
    so = str(tmp_path / "libfpv_alone.so")
    subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + entry.HIPCC_FLAGS + ["-o", so, entry.HIP_SRC], check=True, capture_output=True)
    code = ("import ctypes as C, sys\n"
            "sys.path.insert(0, %r)\n"
            "import torch\n"
            "from fpyv_amd import _lib\n"
            "L = C.CDLL(%r)\n"
            "L.fpv_last_error.restype = C.c_char_p\n"
            "s = _lib.FpvPns()\n"
            "assert L.fpv_sizeof(12) == C.sizeof(_lib.FpvPns)\n"
            "for rc in (L.fpv_pns_eval(C.byref(s), 1, None, None, None), L.fpv_pns_guide(None, None, C.byref(s), None)):\n"
            "    assert rc == -1 and b'linked without csrc/fpv_pns.hip' in L.fpv_last_error(), L.fpv_last_error()\n"
            "print('refused twice')\n") % (REPO, so)
    r = subprocess.run([os.sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "refused twice" in r.stdout, r.stdout + r.stderr
