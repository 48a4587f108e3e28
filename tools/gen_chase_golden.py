#!/usr/bin/env python3
"""Writes tests/golden/g18_chase_calls.npz and g18_chase_loop.npz: captures of the reference's own guidance law
Drone.calculate_needed_force_orientation (src/utils/components.py:258-304), float64, for tests/test_chase_host.py.

The reference is IMPORTED (oracle.gen_golden.import_reference: its pure-Python classes with the display modules stubbed) and run;
nothing of it is copied.  Needs the reference checkout oracle/gen_golden.py names; the committed .npz files are what the tests read.

  g18_chase_calls   64 seeded single calls for each of the four ref_frame x mode pairs, each on a freshly reset drone and PID.  The
                    inputs (p, v, ypr in degrees, the target's centre and radius, the pixel) are rounded through float32.  Drawn
                    so that |v| >= 0.1, the sine of the angle between the reference's own F and the second operand of its first
                    cross product is >= 0.05, about a quarter of the drones fly below tof_effective_distance and about a quarter
                    are beyond the UWB range.
  g18_chase_loop    4 drones (one per ref_frame x mode pair) x 300 steps at fps = 250 of the reference flying its own law against
                    one moving Target: each step the pixel is the projection of the target's centre, the law is called when the
                    target is seen (depth in (0, 15], pixel inside the image) and its result is flown through
                    step(..., rotation_matrix=, thrust_force=); every step records the inputs of the call - the four PID state
                    values before it included - and its outputs.
"""
import contextlib
import copy
import io
import os
import sys

import numpy as np

REPO = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, REPO)
from oracle.gen_golden import import_reference, ref_params  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden")
FPS = 250
PAIRS = [("world", "level"), ("world", "frontarget"), ("drone", "level"), ("drone", "frontarget")]
CASES = 64
MAX_DEPTH = 15.0
# the loop: one target on the reference's circular path, four starts that see it
LOOP_STEPS = 300
LOOP_TARGET = dict(position=[0.0, 0.0, 3.0], radius=0.5, path=dict(radius=25.0, resolution=5500))
LOOP_STARTS = [dict(p=[16.0, -3.0, 4.0], v=[1.0, 0.5, 0.0], ypr=[0.0, 0.0, 20.0]),
               dict(p=[17.0, 4.0, 2.5], v=[0.5, -1.0, 0.2], ypr=[5.0, -5.0, -30.0]),
               dict(p=[15.0, 0.0, 1.5], v=[2.0, 0.0, 0.0], ypr=[0.0, 0.0, 0.0]),
               dict(p=[18.0, -6.0, 6.0], v=[0.0, 1.5, -0.5], ypr=[-5.0, 5.0, 45.0])]
LOOP_ACTION = np.array([-0.1, 0.0, 0.0, 0.0])                  # simulator.py:89


def f32(x):
    return np.asarray(x, dtype=np.float32).astype(np.float64)


def pid_state(pid):
    return np.array([float(pid.integral), float(pid.prev_derivative), float(pid.previous_error), float(bool(pid.is_first))])


def project(cam, c):
    """pixel (x, y) and depth of the world point c through the reference's own projection matrix"""
    h = cam.projection_matrix @ np.append(c, 1.0)
    return h[:2] / h[2], h[2]


def constants(params, drone):
    pid = drone.force_multiplier_pid
    return dict(fps=float(FPS), mass=drone.mass, virtual_drag_coefficient=drone.virtual_drag_coef,
                virtual_lift_coefficient=drone.virtual_lift_coef, tof_effective_distance=float(drone.tof_effective_dist),
                keep_distance=float(drone.keep_distance), UWB_sensor_max_range=float(drone.UWB_sensor_max_range),
                pid_gains=np.array([pid.kP, pid.kI, pid.kD, pid.dt, pid.integral_clip, pid.min_output, pid.max_output,
                                    pid.derivative_transition_rate], dtype=np.float64),
                camera_angle=float(params["camera"]["camera_angle"]), camera_fov=float(params["camera"]["fov"]),
                camera_resolution=np.array(params["camera"]["resolution"], dtype=np.int64),
                camera_position=np.array(params["camera"]["position_relative_to_frame"], dtype=np.float64),
                focal_length=float(drone.camera.focal_length), relative_rotation=np.array(drone.camera.relative_rotation_matrix),
                max_depth=MAX_DEPTH, pairs=np.array(["/".join(p) for p in PAIRS]))


def gen_calls(Drone, Target, params):
    rng = np.random.default_rng(18)
    with contextlib.redirect_stdout(io.StringIO()):
        drone = Drone(copy.deepcopy(params))
    W, H = params["camera"]["resolution"]
    keys = ("p", "v", "ypr", "R", "target", "radius", "pixel", "rot", "force", "pid_after", "pid_error", "pid_derivative")
    rec = {k: [[] for _ in PAIRS] for k in keys}
    for k, (frame, mode) in enumerate(PAIRS):
        n = 0
        while n < CASES:
            low, far = n % 4 == 1, n % 4 == 2                     # a quarter below tof, a quarter beyond the UWB range
            p = f32([rng.uniform(-10, 10), rng.uniform(-10, 10), rng.uniform(0.3, 1.9) if low else rng.uniform(2.1, 10.0)])
            speed = rng.uniform(0.1, 8.0)
            u = rng.normal(size=3)
            v = f32(u / np.linalg.norm(u) * speed)
            radius = float(f32(rng.uniform(0.2, 1.0)))
            rho = rng.uniform(14.5, 30.0) if far else rng.uniform(2.0, 12.0)
            az, el = rng.uniform(-np.pi, np.pi), rng.uniform(-0.3, 0.6)
            c = f32(p + rho * np.array([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)]))
            ypr = f32([rng.uniform(-20, 20), rng.uniform(-20, 20), np.rad2deg(az) + rng.uniform(-30, 30)])
            with contextlib.redirect_stdout(io.StringIO()):
                drone.reset(position=p.copy(), velocity=v.copy(), ypr=ypr.copy())
                centre, depth = project(drone.camera, c)
                pixel = f32(centre + rng.uniform(-5, 5, 2))
                if not (depth > 0 and 0 <= pixel[0] < W and 0 <= pixel[1] < H) or np.linalg.norm(v) < 0.1:
                    continue
                target = Target(c.copy(), radius, 1)
                rot, force = drone.calculate_needed_force_orientation(pixel.copy(), target, ref_frame=frame, mode=mode)
            F = rot[:, 2] * force
            g = np.array([0.0, 0.0, -9.81 * drone.mass])
            b = (drone.rotation_matrix @ g if frame == "drone" else g) if mode == "level" else drone.camera.pixel2direction(pixel)
            sine = np.linalg.norm(np.cross(F, b)) / (np.linalg.norm(F) * np.linalg.norm(b))
            if not sine >= 0.05 or not np.all(np.isfinite(rot)):
                continue
            pid = drone.force_multiplier_pid
            for key, val in (("p", p), ("v", v), ("ypr", ypr), ("R", drone.rotation_matrix.copy()), ("target", c), ("radius", radius),
                             ("pixel", pixel), ("rot", np.array(rot)), ("force", float(force)), ("pid_after", pid_state(pid)),
                             ("pid_error", float(pid.error)), ("pid_derivative", float(pid.derivative))):
                rec[key][k].append(val)
            n += 1
    out = {k: np.asarray(v, dtype=np.float64) for k, v in rec.items()}
    below = float(np.mean(out["p"][..., 2] < drone.tof_effective_dist))
    beyond = float(np.mean(np.linalg.norm(out["p"] - out["target"], axis=-1) - out["radius"] > drone.UWB_sensor_max_range))
    print(f"g18_chase_calls: {below:.2f} of the cases below tof, {beyond:.2f} beyond the UWB range")
    np.savez_compressed(os.path.join(OUT, "g18_chase_calls.npz"), **out, **constants(params, drone))


def gen_loop(Drone, Target, params):
    W, H = params["camera"]["resolution"]
    with contextlib.redirect_stdout(io.StringIO()):
        drones = [Drone(copy.deepcopy(params)) for _ in PAIRS]
        for d, s in zip(drones, LOOP_STARTS):
            d.reset(position=np.array(s["p"]), velocity=np.array(s["v"]), ypr=np.array(s["ypr"]))
    target = Target(np.array(LOOP_TARGET["position"]), LOOP_TARGET["radius"], 1, path=dict(LOOP_TARGET["path"]))
    keys = ("p", "v", "R", "target", "pixel", "depth", "seen", "pid_before", "rot", "force", "pid_after", "distance")
    rec = {k: [] for k in keys}
    wind = np.zeros(3)
    for _ in range(LOOP_STEPS):
        target.update()
        row = {k: [] for k in keys}
        for d, (frame, mode) in zip(drones, PAIRS):
            pixel, depth = project(d.camera, np.asarray(target.position, dtype=np.float64))
            seen = bool(depth > 0 and depth <= MAX_DEPTH and 0 <= pixel[0] < W and 0 <= pixel[1] < H)
            row["p"].append(d.position.copy()); row["v"].append(d.velocity.copy()); row["R"].append(d.rotation_matrix.copy())
            row["target"].append(np.array(target.position, dtype=np.float64)); row["pixel"].append(pixel); row["depth"].append(depth)
            row["seen"].append(float(seen)); row["pid_before"].append(pid_state(d.force_multiplier_pid))
            row["distance"].append(np.linalg.norm(d.position - target.position))
            with contextlib.redirect_stdout(io.StringIO()):
                if seen:
                    rot, force = d.calculate_needed_force_orientation(pixel.copy(), target, ref_frame=frame, mode=mode)
                    d.step(action=LOOP_ACTION.copy(), wind_velocity_vector=wind, object_list=[], rotation_matrix=rot, thrust_force=force)
                else:
                    rot, force = np.full((3, 3), np.nan), np.nan
                    d.step(action=LOOP_ACTION.copy(), wind_velocity_vector=wind, object_list=[])
            row["rot"].append(np.array(rot)); row["force"].append(float(force)); row["pid_after"].append(pid_state(d.force_multiplier_pid))
        for k in keys:
            rec[k].append(row[k])
    out = {k: np.asarray(v, dtype=np.float64) for k, v in rec.items()}                    # [step, drone, ...]
    print(f"g18_chase_loop: seen on {int(out['seen'].sum())} of {out['seen'].size} drone-steps; distance to the target "
          f"{out['distance'][0].round(2)} -> min {out['distance'].min(0).round(2)}")
    np.savez_compressed(os.path.join(OUT, "g18_chase_loop.npz"), **out, radius=float(LOOP_TARGET["radius"]),
                        starts_p=np.array([s["p"] for s in LOOP_STARTS]), starts_v=np.array([s["v"] for s in LOOP_STARTS]),
                        starts_ypr=np.array([s["ypr"] for s in LOOP_STARTS]), action=LOOP_ACTION,
                        target_centre=np.array(LOOP_TARGET["position"]), target_path=np.array([LOOP_TARGET["path"]["radius"], LOOP_TARGET["path"]["resolution"]]),
                        **constants(params, drones[0]))


def main():
    yaml_helper, Drone, _, _ = import_reference()
    from utils.components import Target
    params = ref_params(yaml_helper, FPS)
    gen_calls(Drone, Target, params)
    gen_loop(Drone, Target, params)


if __name__ == "__main__":
    main()
