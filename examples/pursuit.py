#!/usr/bin/env python3
"""The reference simulator's chase loop (/root/reference/src/core/simulator.py:54-110) for N drones with a target EACH, headless:

    targets = generate_targets(...)                       # once
    loop:   [target.update() for target in targets]       # on the device, inside the pursuit call
            rot_mat, force_size = drone.calculate_needed_force_orientation(pixel, targets[idx])     # --guided: the same call
            drone.step(action, ..., rotation_matrix=rot_mat, thrust_force=force_size)

`FpvVecEnv(pursuit=PursuitTask(...))` launches one pursuit kernel after every step: it advances every drone's own target along its
circular path, pays the progress towards it and a capture bonus, respawns a captured target in the spawn box, observes the target in
the drone's body frame and, with --guided, runs the reference's guidance law against that target and feeds the next step's
override.  Without --guided the drones fly hover sticks (a policy would read `env.target_obs`).

Usage:  python examples/pursuit.py --drones 4096 --steps 2000 [--guided]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fpyv_amd import load_params  # noqa: E402
from fpyv_amd.env import FpvVecEnv  # noqa: E402
from fpyv_amd.pursuit import PursuitTask  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--drones", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--fps", type=float, default=250.0)
    ap.add_argument("--guided", action="store_true", help="fly the reference's guidance law against every drone's own target")
    ap.add_argument("--capture", type=float, default=6.5, help="capture distance [m] (the law keeps keep_distance = 6 m)")
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    dev, n = "cuda:0", a.drones
    rng = np.random.default_rng(a.seed)
    params = load_params(fps=a.fps)
    # every drone starts 9..12 m behind the first point of its target's path, nose towards it: the camera sees the target
    centre = rng.uniform([-200, -200, 4], [200, 200, 8], (n, 3)).astype(np.float32)
    phi = np.deg2rad(rng.uniform(-130.0, -50.0, n))
    rho = rng.uniform(9.0, 12.0, n)
    start = centre + np.float32([25.0, 0.0, 0.0]) + np.stack([rho * np.cos(phi), rho * np.sin(phi), rng.uniform(-0.5, 2.0, n)], axis=1)
    ypr = np.stack([np.zeros(n), np.zeros(n), np.rad2deg(phi) + 180.0 + rng.uniform(-15, 15, n)], axis=1)
    task = PursuitTask(targets=dict(centre=centre, radius=0.5, path_radius=25.0), path=dict(radius=25.0, resolution=55000),
                       capture_distance=a.capture, rewards=dict(progress=1.0, capture=10.0),
                       respawn=dict(lo=(-200.0, -200.0, 4.0), hi=(200.0, 200.0, 8.0), radius=(0.4, 0.6), seed=a.seed),
                       respawn_on_done=False, guide=dict(ref_frame="world", mode="level") if a.guided else None)
    env = FpvVecEnv(params, num_envs=n, device=dev, auto_reset=False, pursuit=task, guided=a.guided)
    env.reset(position=start.astype(np.float32), velocity=np.zeros(3), ypr=ypr.astype(np.float32))
    sticks = torch.tensor([0.0, 0.0, 0.0, -0.646], device=dev).expand(n, 4).contiguous()       # hover throttle where not guided
    captures = torch.zeros(n, dtype=torch.int64, device=dev)
    ret = torch.zeros(n, device=dev)

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        _, reward, _, info = env.step(sticks)
        captures += info["target_event"]
        ret += reward
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    dist = env.target_obs[:, 6]
    print(f"{n} drones x {a.steps} steps (dt = {params.dt * 1e3:.1f} ms, {'guided' if a.guided else 'hover sticks'}) in {dt:.3f} s = "
          f"{n * a.steps / dt / 1e6:.1f} M env-steps/s (host loop: one step kernel + one pursuit kernel per step)")
    print(f"captures: {int(captures.sum())} ({float(captures.sum()) / dt:.0f} per second, {int((captures > 0).sum())} drones captured at least once); "
          f"mean distance to the own target {float(dist.mean()):.2f} m; mean return {float(ret.mean()):.2f}; "
          f"finite state: {bool(torch.isfinite(env.obs).all())}")
    env.close()


if __name__ == "__main__":
    main()
