"""The target chase on the host, no GPU: the float64 restatement of the law (tests/chase_law.py) against the reference captures
g18_chase_calls / g18_chase_loop (tools/gen_chase_golden.py) at the oracle tolerance; the library's fp32 lane function
(fpv_chase_eval, the function the kernel runs) against the same captures call by call; the pixel; the cases the build defines where
the reference gives NaN; and the C ABI - version, sizes, every refusal by name, a library built without the unit."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from chase_law import Law, quat_of
from conftest import REPO, load_golden

from fpyv_amd import _lib, load_params
from fpyv_amd.chase import ChaseGuidance

ORACLE_TOL = 1e-12
# fpv_chase_eval (fp32) against the reference captures (float64), inputs narrowed to fp32: the largest error measured over both g18
# files is 6.9e-6 on a matrix entry (the x and y columns carry the fp32 rounding of F divided by the sine of the angle between F and
# the second operand of the cross product, which the reference's own flight of the loop file does not keep large) and 2.5e-7
# relative on the force; the bound is that with a margin of 8 for inputs the captures do not span
FP32_TOL_MATRIX = 8 * 6.9e-6
FP32_TOL_FORCE = 8 * 2.5e-7
# the PID rows after a call, from the number format: positions and centres of the captures are below 32 m, where an fp32 value is
# within 1.9e-6 / 2 of the float64 one per component; the distance, hence the error row, is then within 4e-6 (three components of
# two points and the operations of the norm), the integral row moves by dt times that, and the derivative row is the difference of
# two such errors (the recorded previous error is narrowed on its own) divided by dt and scaled by the filter's rate
FP32_TOL_PID_ERROR = 4e-6
PAIRS = [("world", "level"), ("world", "frontarget"), ("drone", "level"), ("drone", "frontarget")]


@pytest.fixture(scope="module")
def calls():
    return load_golden("g18_chase_calls")


@pytest.fixture(scope="module")
def loop():
    return load_golden("g18_chase_loop")


@pytest.fixture(scope="module")
def params():
    return load_params(fps=250)


def fresh():
    return np.array([0.0, 0.0, 0.0, 1.0])


def rel(a, b):
    """|a - b| relative to the quantity's magnitude"""
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(1.0, float(np.max(np.abs(b)))))


def test_the_captures_are_what_the_issue_asks_for(calls, loop):
    assert [str(x) for x in calls["pairs"]] == ["/".join(p) for p in PAIRS]
    assert calls["p"].shape == (4, 64, 3) and loop["p"].shape == (300, 4, 3)
    for k in ("p", "v", "ypr", "target", "radius", "pixel"):
        assert np.array_equal(calls[k], calls[k].astype(np.float32).astype(np.float64)), k
    assert np.linalg.norm(calls["v"], axis=-1).min() >= 0.1
    below = np.mean(calls["p"][..., 2] < calls["tof_effective_distance"])
    beyond = np.mean(np.linalg.norm(calls["p"] - calls["target"], axis=-1) - calls["radius"] > calls["UWB_sensor_max_range"])
    assert 0.2 <= below <= 0.3 and 0.2 <= beyond <= 0.3
    assert 0 < loop["seen"].sum() < loop["seen"].size                # both branches of simulator.py:104 are flown


def test_the_packaged_parameters_are_the_captures(calls, params):
    """keep_distance, UWB_sensor_max_range, point_and_shoot, camera and the PID's output limits, as load_params derives them"""
    law, ref = Law.from_params(params), Law.from_golden(calls)
    for k in ("f", "w", "h", "vdrag", "vlift", "tof", "keep", "uwb", "kP", "kI", "kD", "dt", "iclip", "lo", "hi", "drate", "max_depth"):
        assert abs(getattr(law, k) - getattr(ref, k)) <= 1e-12 * max(1.0, abs(getattr(ref, k))), k
    assert np.allclose(law.rr, ref.rr, atol=1e-15) and np.allclose(law.rel, ref.rel) and np.allclose(law.g, ref.g, rtol=1e-15)
    assert params.point_and_shoot["ref_frame"] == "world" and params.point_and_shoot["mode"] == "level"


def test_float64_restatement_matches_every_single_call_of_the_reference(calls):
    law = Law.from_golden(calls)
    worst = 0.0
    for k, (frame, mode) in enumerate(PAIRS):
        for i in range(64):
            rot, force, _, seen, st = law(calls["p"][k, i], calls["v"][k, i], calls["R"][k, i], calls["target"][k, i], calls["radius"][k, i],
                                          fresh(), pixel=calls["pixel"][k, i], frame=frame, mode=mode)
            assert seen
            worst = max(worst, rel(rot, calls["rot"][k, i]), rel(force, calls["force"][k, i]), rel(st, calls["pid_after"][k, i]))
            assert st[2] == pytest.approx(calls["pid_error"][k, i], rel=ORACLE_TOL, abs=ORACLE_TOL)
            assert st[1] == pytest.approx(calls["pid_derivative"][k, i], rel=ORACLE_TOL, abs=ORACLE_TOL)
    print(f"restatement vs single calls: {worst:.2e}")
    assert worst <= ORACLE_TOL


def test_float64_restatement_matches_every_step_of_the_reference_loop(loop):
    law = Law.from_golden(loop)
    worst = 0.0
    for t in range(loop["p"].shape[0]):
        for k, (frame, mode) in enumerate(PAIRS):
            pixel, depth, seen = law.project(loop["p"][t, k], loop["R"][t, k], loop["target"][t, k])
            assert seen == bool(loop["seen"][t, k])
            worst = max(worst, rel(depth, loop["depth"][t, k]))
            if seen:            # (an unseen centre may lie in the camera's own plane, where a pixel is the quotient of two roundings)
                worst = max(worst, rel(pixel, loop["pixel"][t, k]))
            rot, force, _, _, st = law(loop["p"][t, k], loop["v"][t, k], loop["R"][t, k], loop["target"][t, k], float(loop["radius"]),
                                       loop["pid_before"][t, k], pixel=loop["pixel"][t, k] if seen else np.full(2, np.nan), frame=frame, mode=mode)
            worst = max(worst, rel(st, loop["pid_after"][t, k]))
            if seen:
                worst = max(worst, rel(rot, loop["rot"][t, k]), rel(force, loop["force"][t, k]))
            else:
                assert np.isnan(force) and np.array_equal(rot, np.eye(3)) and np.isnan(loop["force"][t, k])
    print(f"restatement vs loop: {worst:.2e}")
    assert worst <= ORACLE_TOL


def guidance(params, frame, mode, **kw):
    return ChaseGuidance(params, ref_frame=frame, mode=mode, **kw)


def quats(R):
    return np.array([quat_of(r) for r in R.reshape(-1, 3, 3)])


def test_fp32_host_function_matches_the_reference_captures_call_by_call(calls, loop, params):
    em = ef = 0.0
    ep = np.zeros(4)
    tol_rows = np.array([FP32_TOL_PID_ERROR, 2 * FP32_TOL_PID_ERROR / params.dt * params.force_multiplier_pid["derivative_transition_rate"],
                         FP32_TOL_PID_ERROR, 0.0])
    for k, (frame, mode) in enumerate(PAIRS):
        G = guidance(params, frame, mode)
        # the single calls: one target per case, so one call of the batch function per case
        for i in range(64):
            rot, thrust, _, vis, st = G.evaluate(calls["p"][k, i:i + 1], calls["v"][k, i:i + 1], quats(calls["R"][k, i]),
                                                 (calls["target"][k, i], calls["radius"][k, i]), None, calls["pixel"][k, i:i + 1])
            assert vis[0]
            em = max(em, float(np.abs(rot[0] - calls["rot"][k, i]).max()))
            ef = max(ef, abs(float(thrust[0]) - calls["force"][k, i]) / calls["force"][k, i])
            ep = np.maximum(ep, np.abs(st[:, 0] - calls["pid_after"][k, i]))
        # the loop: every step is fed the reference's recorded inputs and PID state, nothing accumulates
        for t in range(loop["p"].shape[0]):
            seen = bool(loop["seen"][t, k])
            pix = loop["pixel"][t, k:k + 1] if seen else np.full((1, 2), np.nan)
            rot, thrust, _, vis, st = G.evaluate(loop["p"][t, k:k + 1], loop["v"][t, k:k + 1], quats(loop["R"][t, k]),
                                                 (loop["target"][t, k], float(loop["radius"])), loop["pid_before"][t, k].reshape(4, 1), pix)
            assert bool(vis[0]) == seen
            ep = np.maximum(ep, np.abs(st[:, 0] - loop["pid_after"][t, k]))
            if seen:
                em = max(em, float(np.abs(rot[0] - loop["rot"][t, k]).max()))
                ef = max(ef, abs(float(thrust[0]) - loop["force"][t, k]) / loop["force"][t, k])
            else:
                assert np.isnan(thrust[0]) and np.array_equal(rot[0], np.eye(3, dtype=np.float32))
    print(f"fpv_chase_eval vs captures: matrix {em:.2e}, force {ef:.2e} relative, PID rows {ep} (bounds {tol_rows})")
    assert em <= 1e-5 and ef <= 1e-5                                  # a measured error above 1e-5 would be a finding
    assert em <= FP32_TOL_MATRIX and ef <= FP32_TOL_FORCE and np.all(ep <= tol_rows)


# ---- the pixel ----------------------------------------------------------------------------------------------------------
def pixel_scene(law, n=400, seed=3):
    """poses around a target at the origin of the scene, the float64 projection, and which of them keep 1e-3 of the image size
    (and of max_depth) away from every visibility boundary"""
    rng = np.random.default_rng(seed)
    p = rng.uniform([-14, -14, 0.5], [14, 14, 9], (n, 3)).astype(np.float32)
    ypr = rng.uniform([-25, -25, -180], [25, 25, 180], (n, 3))
    from fpyv_amd.params import ypr_to_quat
    q = np.array([ypr_to_quat(*a) for a in ypr]).astype(np.float32)
    c = np.array([1.0, -2.0, 4.0], dtype=np.float32)
    pix, depth, seen, clear = np.zeros((n, 2)), np.zeros(n), np.zeros(n, bool), np.zeros(n, bool)
    for i in range(n):
        qq = q[i].astype(np.float64)
        w, x, y, z = qq / np.linalg.norm(qq)
        R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                      [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
        pix[i], depth[i], seen[i] = law.project(p[i].astype(np.float64), R, c.astype(np.float64))
        with np.errstate(all="ignore"):
            edges = [abs(depth[i]), abs(depth[i] - law.max_depth)] if not (depth[i] > 1e-3 * law.max_depth) else \
                    [depth[i], abs(depth[i] - law.max_depth), *(abs(pix[i, 0] - e) * law.max_depth / law.w for e in (0.0, law.w)),
                     *(abs(pix[i, 1] - e) * law.max_depth / law.h for e in (0.0, law.h))]
        clear[i] = min(edges) >= 1e-3 * law.max_depth
    return p, q, c, pix, depth, seen, clear


def test_track_pixel_matches_the_float64_projection_and_visible_is_exact(params):
    law = Law.from_params(params)
    p, q, c, pix, _, seen, clear = pixel_scene(law)
    _, thrust, got, vis, _ = guidance(params, "world", "level").evaluate(p, np.ones_like(p), q, (c, 0.5))
    assert clear.sum() > 300 and 40 < (seen & clear).sum() < clear.sum() - 40
    assert np.array_equal(vis[clear], seen[clear])
    s = seen & clear
    err = np.abs(got[s] - pix[s]).max(axis=0) / np.array([law.w, law.h])
    print(f"pixel vs float64 projection, relative to the image size: {err}")
    assert err.max() <= FP32_TOL_MATRIX
    assert np.all(np.isnan(got[~vis])) and np.all(np.isnan(thrust[~vis])) and np.all(np.isfinite(thrust[vis]))


# a level drone at the origin looking along +x (the camera looks 35 degrees up, 60 degrees to either side): a target's centre and
# the ONE visibility condition it fails, as the float64 projection sees it
UNSEEN = {"behind": ([-4.1, 0, -2.87], "depth > 0"), "beyond max_depth": ([30, 0, 21], "depth <= max_depth"), "left": ([1, 8, 1], "u < W"),
          "right": ([1, -8, 1], "u >= 0"), "above": ([-0.5, 0, 9], "v >= 0"), "below": ([2, 0, -1.5], "v < H")}


@pytest.mark.parametrize("where", list(UNSEEN))
def test_an_unseen_target_leaves_the_drone_unguided_and_its_pid_untouched(params, where):
    G, law = guidance(params, "world", "level"), Law.from_params(params)
    c, fails = UNSEEN[where]
    # only the condition the label names fails
    (u, v), depth, seen = law.project(np.zeros(3), np.eye(3), np.array(c, dtype=np.float64))
    holds = {"depth > 0": depth > 0, "depth <= max_depth": depth <= law.max_depth, "u >= 0": u >= 0, "u < W": u < law.w, "v >= 0": v >= 0,
             "v < H": v < law.h}
    assert not seen and [k for k, ok in holds.items() if not ok] == [fails], (where, depth, u, v)
    st = np.array([[0.3], [-0.2], [1.5], [0.0]], dtype=np.float32)
    rot, thrust, pix, vis, after = G.evaluate([[0, 0, 0]], [[1, 0, 0]], [[1, 0, 0, 0]], (c, 0.5), st)
    assert not vis[0] and np.isnan(thrust[0]) and np.all(np.isnan(pix))
    assert np.array_equal(rot[0], np.eye(3, dtype=np.float32)) and np.array_equal(after, st)
    # ... and the same drone sees a target in front of it
    _, thrust, pix, vis, after = G.evaluate([[0, 0, 0]], [[1, 0, 0]], [[1, 0, 0, 0]], ([6, 0, 4], 0.5), st)
    assert vis[0] and np.isfinite(thrust[0]) and after[3, 0] == 0.0 and not np.array_equal(after, st)


def test_a_nan_pixel_is_an_unseen_target_and_640_by_480_is_accepted(params):
    G = guidance(params, "world", "level")
    assert G.camera.resolution == (640, 480) and G.derive().width == 640
    pixel = np.array([[320.0, 240.0], [np.nan, 100.0], [100.0, np.nan]])
    rot, thrust, pix, vis, st = G.evaluate(np.zeros((3, 3)), np.ones((3, 3)), np.tile([1.0, 0, 0, 0], (3, 1)), ([6, 0, 4], 0.5), None, pixel)
    assert list(vis) == [True, False, False] and np.isfinite(thrust[0]) and np.all(np.isnan(thrust[1:]))
    assert np.array_equal(pix[0], pixel[0].astype(np.float32)) and np.all(np.isnan(pix[1:]))
    assert list(st[3]) == [0.0, 1.0, 1.0]


# ---- defined where the reference gives NaN ------------------------------------------------------------------------------
def orthonormal(rot, thrust, F=None):
    assert np.all(np.isfinite(rot)) and np.isfinite(thrust)
    assert np.abs(rot.T.astype(np.float64) @ rot.astype(np.float64) - np.eye(3)).max() <= 1e-6
    if F is not None:
        assert np.abs(rot[:, 2] - F / np.linalg.norm(F)).max() <= 1e-6


@pytest.mark.parametrize("frame,mode", PAIRS)
def test_zero_velocity_gives_zero_drag_and_a_finite_frame(params, frame, mode):
    law = Law.from_params(params)
    p, c = np.array([0.0, 0.0, 5.0]), np.array([6.0, 1.0, 7.0])
    rot, thrust, _, vis, _ = guidance(params, frame, mode).evaluate([p], [[0, 0, 0]], [[1, 0, 0, 0]], (c, 0.5))
    want, force, _, _, _ = law(p, np.zeros(3), np.eye(3), c, 0.5, fresh(), frame=frame, mode=mode)
    assert vis[0]
    orthonormal(rot[0], thrust[0], want[:, 2] * force)
    assert np.abs(rot[0] - want).max() <= FP32_TOL_MATRIX and abs(thrust[0] - force) <= FP32_TOL_FORCE * force


def test_force_parallel_to_gravity_takes_the_fallback_axis(params):
    """level: a pixel whose direction is straight up and no velocity: F = m d - g is vertical, F x g = 0"""
    law = Law.from_params(params)
    up = law.rr.T @ np.array([0.0, 0.0, 1.0])                          # the camera-frame direction of world +z for a level drone
    pixel = np.array([[law.f * up[0] / up[2] + law.w / 2, law.f * up[1] / up[2] + law.h / 2]])
    rot, thrust, _, vis, _ = guidance(params, "world", "level").evaluate([[0, 0, 5]], [[0, 0, 0]], [[1, 0, 0, 0]], ([0, 0, 9], 0.5), None, pixel)
    assert vis[0]
    orthonormal(rot[0], thrust[0], np.array([0.0, 0.0, 1.0]))
    assert np.abs(rot[0][:, 1] - [0.0, 1.0, 0.0]).max() <= 1e-6          # y = F x (1, 0, 0) normalised, F along +z


def test_force_parallel_to_the_direction_takes_the_fallback_axis_in_frontarget(params):
    """frontarget with the target straight below, no velocity, above tof: F = m d - g with d = (0, 0, -1) is parallel to d"""
    law = Law.from_params(params)
    q = np.array([[np.cos(np.pi / 4), 0.0, np.sin(np.pi / 4), 0.0]])        # nose down: the camera's view holds the nadir
    R = np.array([[0.0, 0.0, 1.0], [0.0, 1.0, 0.0], [-1.0, 0.0, 0.0]])
    down = law.rr.T @ (R.T @ np.array([0.0, 0.0, -1.0]))
    assert down[2] > 0
    pixel = np.array([[law.f * down[0] / down[2] + law.w / 2, law.f * down[1] / down[2] + law.h / 2]])
    rot, thrust, _, vis, _ = guidance(params, "world", "frontarget").evaluate([[0, 0, 9]], [[0, 0, 0]], q, ([0, 0, 3], 0.5), None, pixel)
    assert vis[0]
    want, force, _, _, _ = law([0, 0, 9], np.zeros(3), R, [0, 0, 3], 0.5, fresh(), pixel=pixel[0], frame="world", mode="frontarget")
    F = want[:, 2] * force
    assert abs(F[0]) <= 1e-9 * force and abs(F[1]) <= 1e-9 * force           # F is vertical, like d
    orthonormal(rot[0], thrust[0], F)
    assert np.abs(rot[0] - want).max() <= FP32_TOL_MATRIX and abs(thrust[0] - force) <= FP32_TOL_FORCE * force
    assert abs(abs(rot[0][1, 1]) - 1.0) <= 1e-6                            # y along the world y axis: F x (1, 0, 0)


# ---- the C ABI -------------------------------------------------------------------------------------------------------------
def test_abi_version_and_struct_sizes():
    L = _lib.lib()
    assert L.fpv_abi_version() == 9 == _lib.FPV_ABI_VERSION
    assert L.fpv_sizeof(0) == C.sizeof(_lib.FpvParams) == 688 and L.fpv_sizeof(1) == C.sizeof(_lib.FpvBuffers) == 200
    assert L.fpv_sizeof(8) == C.sizeof(_lib.FpvChase) == 328
    assert L.fpv_sizeof(9) < 0 and b"7 = fpv_depth_render_t, 8 = fpv_chase_t" in L.fpv_last_error()
    import __graft_entry__ as entry
    assert entry.HIP_SRCS_BUILD == entry.HIP_SRCS_ALL + [os.path.join(REPO, "fpyv_amd", "csrc", "fpv_chase.hip")]
    assert all(hasattr(L, s) for s in ("fpv_chase_derive", "fpv_chase_guide", "fpv_chase_eval")) and "fpv_chase_guide" in _lib.EXPORTS


def refused(s, n=2, what=None, p=None, v=None, q=None):
    L = _lib.lib()
    zeros = np.zeros((n, 4), dtype=np.float32)
    arg = lambda a: (zeros if a is None else a).ctypes.data  # noqa: E731
    rc = L.fpv_chase_eval(C.byref(s) if s is not None else None, n, arg(p) if p is not False else None, arg(v) if v is not False else None,
                          arg(q) if q is not False else None)
    msg = L.fpv_last_error().decode()
    assert rc < 0 and (what is None or what in msg), (rc, msg)
    return rc


def test_every_refusal_names_its_reason(params):
    L = _lib.lib()
    G = guidance(params, "world", "level")
    n = 2
    st, rot, thrust = np.zeros((4, n), dtype=np.float32), np.zeros((n, 9), dtype=np.float32), np.zeros(n, dtype=np.float32)

    def good():
        s = G.derive(([1, 2, 3], 0.5))
        s.pid_state, s.pid_ld, s.rotation, s.thrust = st.ctypes.data, n, rot.ctypes.data, thrust.ctypes.data
        return s

    zeros = np.zeros((n, 4), dtype=np.float32)
    assert L.fpv_chase_eval(C.byref(good()), n, zeros.ctypes.data, zeros.ctypes.data, zeros.ctypes.data) == 0
    cases = [("struct_size", 0, "struct_size"), ("width", 0, "width and height"), ("height", 20000, "width and height"),
             ("ref_frame", 2, "unknown ref_frame"), ("mode", -1, "unknown mode"), ("focal_length", float("nan"), "focal_length"),
             ("max_depth", 0.0, "max_depth"), ("max_depth", float("inf"), "max_depth"), ("mass", -1.0, "mass"),
             ("virtual_drag_coefficient", float("nan"), "virtual_drag_coefficient"), ("virtual_lift_coefficient", float("inf"), "virtual_lift_coefficient"),
             ("tof_effective_distance", float("nan"), "tof_effective_distance"), ("keep_distance", float("nan"), "keep_distance"),
             ("UWB_sensor_max_range", float("inf"), "UWB_sensor_max_range"), ("target_radius", -1.0, "radius"),
             ("pid_state", None, "pid_state is null"), ("rotation", None, "rotation is null"), ("thrust", None, "thrust is null"),
             ("pid_ld", 1, "pid_ld"), ("rotation", rot.ctypes.data + 2, "4-byte aligned"), ("pixel", rot.ctypes.data + 4, "8-byte aligned"),
             ("pixel_out", rot.ctypes.data + 4, "8-byte aligned")]
    for field, value, what in cases:
        s = good()
        setattr(s, field, value)
        refused(s, n, what)
    s = good(); s.relative_rotation[4] = float("nan"); refused(s, n, "relative_rotation")
    s = good(); s.target[1] = float("inf"); refused(s, n, "target")
    s = good(); s.pid.struct_size = 8; refused(s, n, "pid.struct_size")
    s = good(); s.pid.dt = 0.0; refused(s, n, "dt must be positive")
    s = good(); s.pid.kI = float("nan"); refused(s, n, "PID constant")
    s = good(); s.pid.min_output = 2.0; s.pid.max_output = 1.0; refused(s, n, "min_output <= max_output")
    refused(None, n, "null argument")
    refused(good(), 0, "n must be positive")
    refused(good(), n, "null argument", v=False)
    # the handle's refusals that need no device
    assert L.fpv_chase_guide(None, None, C.byref(good()), None) < 0 and b"null handle" in L.fpv_last_error()
    # derive
    cam, out = _lib.FpvCamera(), _lib.FpvChase()
    cam.pitch_deg, cam.fov_deg, cam.width, cam.height = 35.0, 120.0, 640, 480
    assert L.fpv_chase_derive(C.byref(cam), C.byref(out)) == 0 and abs(out.focal_length - 320 / np.tan(np.pi / 3)) < 1e-12
    for field, value, what in (("width", 0, "width and height"), ("height", 16385, "width and height"), ("fov_deg", 180.0, "fov"),
                               ("pitch_deg", float("nan"), "pitch")):
        bad = _lib.FpvCamera.from_buffer_copy(cam)
        setattr(bad, field, value)
        assert L.fpv_chase_derive(C.byref(bad), C.byref(out)) < 0 and what.encode() in L.fpv_last_error()
    assert L.fpv_chase_derive(None, C.byref(out)) < 0
    with pytest.raises(ValueError, match="Unknown reference frame"):
        ChaseGuidance(params, ref_frame="camera")
    with pytest.raises(ValueError, match="Unknown mode"):
        ChaseGuidance(params, mode="sideways")


def test_a_library_built_without_the_unit_refuses_by_name(tmp_path):
    """csrc/fpv_hip.hip alone still builds and loads; fpv_chase_guide and fpv_chase_eval say what is missing (a child process: this
    one has the full library loaded)"""
    import __graft_entry__ as entry
    so = str(tmp_path / "libfpv_alone.so")
    subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + entry.HIPCC_FLAGS + ["-o", so, entry.HIP_SRC], check=True, capture_output=True)
    code = ("import ctypes as C, sys\n"
            "sys.path.insert(0, %r)\n"
            "import torch\n"
            "from fpyv_amd import _lib\n"
            "L = C.CDLL(%r)\n"
            "L.fpv_last_error.restype = C.c_char_p\n"
            "s = _lib.FpvChase()\n"
            "assert L.fpv_sizeof(8) == C.sizeof(_lib.FpvChase)\n"
            "for rc in (L.fpv_chase_eval(C.byref(s), 1, None, None, None), L.fpv_chase_guide(None, None, C.byref(s), None)):\n"
            "    assert rc == -1 and b'linked without csrc/fpv_chase.hip' in L.fpv_last_error(), L.fpv_last_error()\n"
            "print('refused twice')\n") % (REPO, so)
    r = subprocess.run([os.sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "refused twice" in r.stdout, r.stdout + r.stderr


# ---- the closed loop the GPU test flies, in float64 on the CPU first ----------------------------------------------------------
def test_the_float64_law_flown_through_the_oracle_override_closes_in_on_the_target(params):
    """tests/test_gpu_chase.py's scenario (chase_law.chase_starts, CHASE_TARGET) with the restatement and the oracle's guided step:
    the guided drones' median closest approach is smaller than that of the same drones left on their hover sticks"""
    from chase_law import CHASE_TARGET, HOVER_STICKS, chase_starts
    from fpyv_amd.objects import Target
    from oracle import oracle
    law, n = Law.from_params(params), 6
    pos, ypr = (x[:n] for x in chase_starts(256))                          # the first six of the GPU test's own 256 starts

    def fly(guided):
        target = Target(CHASE_TARGET["position"], CHASE_TARGET["radius"], path=dict(CHASE_TARGET["path"]))
        state = oracle.drone_initial_state(n, pos.astype(np.float64), np.zeros(3), ypr.astype(np.float64))
        pid, closest = np.tile(fresh(), (n, 1)), np.full(n, np.inf)
        for _ in range(600):
            target.update()
            c = np.asarray(target.position, dtype=np.float64)
            for i in range(n):
                closest[i] = min(closest[i], np.linalg.norm(state[i, :3] - c))
                rot, force = np.eye(3), np.nan
                if guided:
                    rot, force, _, _, pid[i] = law(state[i, :3], state[i, 3:6], state[i, 6:15].reshape(3, 3), c, target.radius, pid[i])
                oracle.drone_run_guided(params, state[i], HOVER_STICKS[None], rot[None], np.array([force]))
        assert np.all(np.isfinite(state))
        return closest

    guided, hover = fly(True), fly(False)
    print(f"median closest approach: guided {np.median(guided):.2f} m, hover sticks {np.median(hover):.2f} m")
    assert np.median(guided) < np.median(hover)
