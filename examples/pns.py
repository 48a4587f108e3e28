#!/usr/bin/env python3
"""Point and shoot as an action space: N drones, a target EACH, steered by the four commands of the reference's
`Drone.point_and_shoot(pixel, action, ref_frame, mode)` (/root/reference/src/utils/components.py:312-381), headless:

    loop:   rot_mat, force_size = drone.point_and_shoot(pixel, action)          # one kernel for all drones
            drone.step(sticks, ..., rotation_matrix=rot_mat, thrust_force=force_size)
            [target.update() for target in targets]                              # on the device, inside the pursuit call

`FpvVecEnv(pursuit=PursuitTask(...), assist=PointAndShoot(...))` takes the commands as its action: action[1] is where on the image
(vertical axis, -1..1) the target is to be held, action[2:] a virtual offset of the target in half-images.  Here every drone flies
one constant command; a learner would put its policy in its place.  Prints the captures per second.

Usage:  python examples/pns.py --drones 4096 --steps 2000 [--command 0 -0.2 0 0]
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
from fpyv_amd.pns import PointAndShoot  # noqa: E402
from fpyv_amd.pursuit import PursuitTask  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--drones", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--fps", type=float, default=250.0)
    ap.add_argument("--command", type=float, nargs=4, default=[0.0, -0.2, 0.0, 0.0], help="the constant action of every drone")
    ap.add_argument("--capture", type=float, default=2.0, help="capture distance [m]")
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
                       respawn=dict(lo=(-200.0, -200.0, 4.0), hi=(200.0, 200.0, 8.0), radius=(0.4, 0.6), seed=a.seed), respawn_on_done=False)
    env = FpvVecEnv(params, num_envs=n, device=dev, auto_reset=False, pursuit=task, assist=PointAndShoot(params),
                    assist_sticks=(0.0, 0.0, 0.0, -0.646))                                   # hover throttle where not guided
    env.reset(position=start.astype(np.float32), velocity=np.zeros(3), ypr=ypr.astype(np.float32))
    command = torch.tensor(a.command, dtype=torch.float32, device=dev).expand(n, 4).contiguous()
    captures = torch.zeros(n, dtype=torch.int64, device=dev)
    guided = torch.zeros((), dtype=torch.int64, device=dev)
    limited = torch.zeros((), dtype=torch.int64, device=dev)

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        _, _, _, info = env.step(command)
        captures += info["target_event"]
        guided += torch.isfinite(env.batch._pns_out["thrust"]).sum()
        limited += (env.batch.thrust_limited > 0).sum()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    dist = env.target_obs[:, 6]
    print(f"{n} drones x {a.steps} steps (dt = {params.dt * 1e3:.1f} ms, command {a.command}) in {dt:.3f} s = "
          f"{n * a.steps / dt / 1e6:.1f} M env-steps/s (host loop: one law kernel + one step kernel + one pursuit kernel per step)")
    print(f"captures: {int(captures.sum())} ({float(captures.sum()) / dt:.0f} per second, {int((captures > 0).sum())} drones captured at least once); "
          f"guided drone-steps {int(guided) / (n * a.steps):.3f}, thrust-limited {int(limited) / (n * a.steps):.4f}; "
          f"mean distance to the own target {float(dist.mean()):.2f} m; finite state: {bool(torch.isfinite(env.obs).all())}")
    env.close()


if __name__ == "__main__":
    main()
