#!/usr/bin/env python3
"""Writes tests/golden/g21_pns_calls.npz and g21_pns_loop.npz: captures of the reference's own steered guidance law
Drone.point_and_shoot (src/utils/components.py:312-381), float64, for tests/test_pns_host.py.

The reference is IMPORTED (oracle.gen_golden.import_reference: its pure-Python classes with the display modules stubbed) and run;
nothing of it is copied.  Needs the reference checkout oracle/gen_golden.py names; the committed .npz files are what the tests read.

The reference's thrust-limit loop (:358-366) does not return when |min_output d + B| > max_throttle_in_force (d = dir2target,
B = virtual drag + virtual lift - gravity).  Before every call this script forms d and B from the reference's own camera and
attributes and SKIPS such a draw - and a draw with Fmax < |F(m0)| <= Fmax (1 + 2e-4), where the loop's first `x 0.9999` step can end it
below the limit the closed form returns.  Every call also runs under an alarm.

  g21_pns_calls   64 seeded single calls for each of the four ref_frame x mode pairs, each on a freshly reset drone.  The inputs (p,
                  v, ypr in degrees, the pixel, the action) are rounded through float32.  |v| >= 0.1; the sine between F and the
                  second operand of the first cross product >= 0.05; a quarter of the drones below tof_effective_distance with
                  v.z < 0; a quarter with the thrust limit binding (drawn at 12..25 m/s, the others at 0.1..8 m/s and not binding);
                  actions uniform in [-1, 1]^4.
  g21_pns_loop    4 drones (one per pair) x 300 steps at fps = 250 of the reference flying its own law against one moving Target
                  under one fixed non-zero command per drone: each step the pixel is the projection of the target's centre, the law
                  is called when the target is seen and its result is flown through step(..., rotation_matrix=, thrust_force=);
                  every step records the inputs of the call - the PID state and prev_pixel before it included - and its outputs.
"""
import contextlib
import copy
import io
import os
import signal
import sys

import numpy as np

REPO = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
from oracle.gen_golden import import_reference, ref_params  # noqa: E402
from gen_chase_golden import FPS, PAIRS, MAX_DEPTH, f32, pid_state, project, constants  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden")
CASES = 64
BAND = 2e-4
LOOP_STEPS = 300
LOOP_TARGET = dict(position=[0.0, 0.0, 3.0], radius=0.5, path=dict(radius=25.0, resolution=5500))
LOOP_STARTS = [dict(p=[16.0, -3.0, 4.0], v=[1.0, 0.5, 0.0], ypr=[0.0, 0.0, 20.0]),
               dict(p=[17.0, 4.0, 2.5], v=[0.5, -1.0, 0.2], ypr=[5.0, -5.0, -30.0]),
               dict(p=[15.0, 0.0, 1.5], v=[2.0, 0.0, -0.3], ypr=[0.0, 0.0, 0.0]),
               dict(p=[18.0, -6.0, 6.0], v=[0.0, 1.5, -0.5], ypr=[-5.0, 5.0, 45.0])]
LOOP_COMMANDS = np.array([[0.3, -0.2, 0.1, 0.05], [-0.5, 0.1, -0.15, 0.1], [0.2, 0.3, 0.05, -0.1], [0.0, -0.4, 0.2, 0.2]])
LOOP_STICKS = np.array([-0.1, 0.0, 0.0, 0.0])                  # simulator.py:89


def prev_pixel(drone):
    return np.full(2, np.nan) if drone.prev_pixel is None else np.array(drone.prev_pixel, dtype=np.float64)


def foresee(drone, pixel, action, frame):
    """(d, B, gravity, |F(m0)|, |F(min_output)|) of the call point_and_shoot(pixel, action) would make, from the reference's own
    camera, attributes and (a copy of) its PID - so that a call that would not return is never made"""
    W, H = drone.camera.resolution
    pix = pixel + action[2:] * np.array([W, H]) / 2
    d = drone.camera.pixel2direction(pix)
    v, R = drone.velocity, drone.rotation_matrix
    g = np.array([0.0, 0.0, -9.81 * drone.mass])
    s = np.linalg.norm(v)
    if frame == "drone":
        g, w = R @ g, R @ v
    else:
        w = v
    k = (w / s) @ d
    drag = drone.virtual_drag_coef * (-(k - 1) / 2 * -w * s)
    lift = (drone.position[2] < drone.tof_effective_dist) * -(drone.tof_effective_dist - drone.position[2]) * drone.virtual_lift_coef * g * -min(v[2], 0.0)
    B = drag + lift - g
    pid = copy.deepcopy(drone.force_multiplier_pid)
    m0 = pid(pix[1], float(int(H / 2 * (1 + action[1]))))
    return d, B, g, np.linalg.norm(m0 * d + B), np.linalg.norm(pid.min_output * d + B)


def returns(drone, f0, fmin):
    """whether the reference's call returns, and with a result the closed form shares"""
    fmax = drone.max_throttle_in_force
    return not fmin > fmax and not fmax * (1 - 1e-9) < f0 <= fmax * (1 + BAND)


def call(drone, pixel, action, frame, mode):
    signal.alarm(60)
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            return drone.point_and_shoot(pixel.copy(), action.copy(), ref_frame=frame, mode=mode)
    finally:
        signal.alarm(0)


def pns_constants(params, drone, model_xy):
    thrust = drone.n_motors * drone.motor_test_report["Thrust"].values / 1000 * drone.gravity          # components.py:134-137
    throttle = drone.motor_test_report["Throttle"].values
    return dict(constants(params, drone), max_throttle_in_force=float(drone.max_throttle_in_force),
                min_throttle_in_force=float(drone.min_throttle_in_force), thrust2throttle_poly=np.array(model_xy(thrust, throttle).coeffs))


def gen_calls(Drone, params, model_xy):
    rng = np.random.default_rng(21)
    with contextlib.redirect_stdout(io.StringIO()):
        drone = Drone(copy.deepcopy(params))
    W, H = params["camera"]["resolution"]
    fmax = drone.max_throttle_in_force
    keys = ("p", "v", "ypr", "R", "pixel", "action", "rot", "force", "throttle", "pid_after", "pid_error", "pid_derivative", "prev_pixel",
            "pixel_velocity", "entered")
    rec = {k: [[] for _ in PAIRS] for k in keys}
    skipped = 0
    for k, (frame, mode) in enumerate(PAIRS):
        n = 0
        while n < CASES:
            low, bind = n % 4 == 1, n % 4 == 2                    # a quarter below tof sinking, a quarter with the limit binding
            p = f32([rng.uniform(-10, 10), rng.uniform(-10, 10), rng.uniform(0.3, 1.9) if low else rng.uniform(2.1, 10.0)])
            speed = rng.uniform(12.0, 25.0) if bind else rng.uniform(0.1, 8.0)
            u = rng.normal(size=3)
            if low:
                u[2] = -abs(u[2])
            v = f32(u / np.linalg.norm(u) * speed)
            ypr = f32([rng.uniform(-20, 20), rng.uniform(-20, 20), rng.uniform(-180, 180)])
            pixel = f32([rng.uniform(0, W), rng.uniform(0, H)])
            action = f32(rng.uniform(-1, 1, 4))
            with contextlib.redirect_stdout(io.StringIO()):
                drone.reset(position=p.copy(), velocity=v.copy(), ypr=ypr.copy())
            if np.linalg.norm(v) < 0.1:
                continue
            d, B, g, f0, fmin = foresee(drone, pixel, action, frame)
            if not returns(drone, f0, fmin):
                skipped += 1
                continue
            entered = bool(f0 > fmax)
            if entered != bind:
                continue
            rot, force = call(drone, pixel, action, frame, mode)
            F = rot[:, 2] * force
            b = g if mode == "level" else d
            sine = np.linalg.norm(np.cross(F, b)) / (np.linalg.norm(F) * np.linalg.norm(b))
            if not sine >= 0.05 or not np.all(np.isfinite(rot)):
                continue
            assert abs(force - (fmax if entered else f0)) <= 1e-9 * fmax, (force, f0, fmax)
            pid = drone.force_multiplier_pid
            for key, val in (("p", p), ("v", v), ("ypr", ypr), ("R", drone.rotation_matrix.copy()), ("pixel", pixel), ("action", action),
                             ("rot", np.array(rot)), ("force", float(force)), ("throttle", float(drone.thrust2throttle(force))),
                             ("pid_after", pid_state(pid)), ("pid_error", float(pid.error)), ("pid_derivative", float(pid.derivative)),
                             ("prev_pixel", prev_pixel(drone)), ("pixel_velocity", np.array(drone.pixel_velocity, dtype=np.float64)),
                             ("entered", float(entered))):
                rec[key][k].append(val)
            n += 1
    out = {k: np.asarray(v, dtype=np.float64) for k, v in rec.items()}
    sinking = float(np.mean((out["p"][..., 2] < drone.tof_effective_dist) & (out["v"][..., 2] < 0)))
    print(f"g21_pns_calls: {sinking:.2f} of the cases below tof with v.z < 0, {out['entered'].mean():.2f} with the limit binding; "
          f"{skipped} draws skipped because the reference would not return (or would stop inside the {BAND:g} band)")
    np.savez_compressed(os.path.join(OUT, "g21_pns_calls.npz"), **out, **pns_constants(params, drone, model_xy))


def gen_loop(Drone, Target, params, model_xy):
    W, H = params["camera"]["resolution"]
    with contextlib.redirect_stdout(io.StringIO()):
        drones = [Drone(copy.deepcopy(params)) for _ in PAIRS]
        for d, s in zip(drones, LOOP_STARTS):
            d.reset(position=np.array(s["p"]), velocity=np.array(s["v"]), ypr=np.array(s["ypr"]))
    target = Target(np.array(LOOP_TARGET["position"]), LOOP_TARGET["radius"], 1, path=dict(LOOP_TARGET["path"]))
    keys = ("p", "v", "R", "target", "pixel", "depth", "seen", "pid_before", "prev_pixel_before", "rot", "force", "throttle", "pid_after",
            "prev_pixel_after", "pixel_velocity", "entered", "distance")
    rec = {k: [] for k in keys}
    wind = np.zeros(3)
    for t in range(LOOP_STEPS):
        target.update()
        row = {k: [] for k in keys}
        for d, (frame, mode), command in zip(drones, PAIRS, LOOP_COMMANDS):
            pixel, depth = project(d.camera, np.asarray(target.position, dtype=np.float64))
            seen = bool(depth > 0 and depth <= MAX_DEPTH and 0 <= pixel[0] < W and 0 <= pixel[1] < H)
            row["p"].append(d.position.copy()); row["v"].append(d.velocity.copy()); row["R"].append(d.rotation_matrix.copy())
            row["target"].append(np.array(target.position, dtype=np.float64)); row["pixel"].append(pixel); row["depth"].append(depth)
            row["seen"].append(float(seen)); row["pid_before"].append(pid_state(d.force_multiplier_pid))
            row["prev_pixel_before"].append(prev_pixel(d))
            row["distance"].append(np.linalg.norm(d.position - target.position))
            entered = False
            if seen:
                _, _, _, f0, fmin = foresee(d, pixel, command, frame)
                if not returns(d, f0, fmin):
                    raise SystemExit(f"g21_pns_loop: step {t}, pair {frame}/{mode}: the reference would not return - choose another start")
                entered = bool(f0 > d.max_throttle_in_force)
                rot, force = call(d, pixel, command, frame, mode)
                throttle, vel = float(d.thrust2throttle(force)), np.array(d.pixel_velocity, dtype=np.float64)
                with contextlib.redirect_stdout(io.StringIO()):
                    d.step(action=LOOP_STICKS.copy(), wind_velocity_vector=wind, object_list=[], rotation_matrix=rot, thrust_force=force)
            else:
                rot, force, throttle, vel = np.full((3, 3), np.nan), np.nan, np.nan, np.full(2, np.nan)
                with contextlib.redirect_stdout(io.StringIO()):
                    d.step(action=LOOP_STICKS.copy(), wind_velocity_vector=wind, object_list=[])
            row["rot"].append(np.array(rot)); row["force"].append(float(force)); row["throttle"].append(throttle)
            row["pid_after"].append(pid_state(d.force_multiplier_pid)); row["prev_pixel_after"].append(prev_pixel(d))
            row["pixel_velocity"].append(vel); row["entered"].append(float(entered))
        for k in keys:
            rec[k].append(row[k])
    out = {k: np.asarray(v, dtype=np.float64) for k, v in rec.items()}                    # [step, drone, ...]
    print(f"g21_pns_loop: seen on {int(out['seen'].sum())} of {out['seen'].size} drone-steps, the limit binding on {int(out['entered'].sum())}; "
          f"distance to the target {out['distance'][0].round(2)} -> min {out['distance'].min(0).round(2)}")
    np.savez_compressed(os.path.join(OUT, "g21_pns_loop.npz"), **out, radius=float(LOOP_TARGET["radius"]),
                        starts_p=np.array([s["p"] for s in LOOP_STARTS]), starts_v=np.array([s["v"] for s in LOOP_STARTS]),
                        starts_ypr=np.array([s["ypr"] for s in LOOP_STARTS]), commands=LOOP_COMMANDS, sticks=LOOP_STICKS,
                        target_centre=np.array(LOOP_TARGET["position"]), target_path=np.array([LOOP_TARGET["path"]["radius"], LOOP_TARGET["path"]["resolution"]]),
                        **pns_constants(params, drones[0], model_xy))


def main():
    yaml_helper, Drone, _, _ = import_reference()
    from utils.components import Target
    from utils.flight_time_calculator import model_xy
    params = ref_params(yaml_helper, FPS)
    gen_calls(Drone, params, model_xy)
    gen_loop(Drone, Target, params, model_xy)


if __name__ == "__main__":
    main()
