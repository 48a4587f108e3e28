#!/usr/bin/env python3
"""Obstacle avoidance with the range sensor: N drones fly forward through a world of two cylinders, a sphere and the ground,
steered by a hand-written rule on a 9-ray fan (tilted up a little, so that a drone leaning forward does not take the ground for a
wall) - `env.ranges`, which a scan kernel writes after every step (include/fpv_abi.h "Range scan").  The same flight is flown twice, once with the rule blind (every ray reads max_range), and the crashes
of both are printed.

    python examples/obstacle_avoidance.py --drones 4096 --steps 1200
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fpyv_amd import load_params, rays  # noqa: E402
from fpyv_amd.env import FpvVecEnv  # noqa: E402
from fpyv_amd.objects import Cylinder, Ground, Target  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--drones", type=int, default=4096)
ap.add_argument("--steps", type=int, default=1200)
ap.add_argument("--speed", type=float, default=4.0)
a = ap.parse_args()
dev = torch.device("cuda:0")
p = load_params(fps=200, ceiling=100.0)
world = [Target([1.5, -6.0, 3.0], 0.8), Cylinder([3.0, 0.0, 0.0], 1.0, 5.0), Cylinder([-2.0, 2.5, 0.0], 0.6, 1.5), Ground()]
n, RMAX, Z0 = a.drones, 6.0, 2.5
rng = np.random.default_rng(0)
start = np.stack([np.full(n, -10.0), rng.uniform(-7.0, 4.0, n), Z0 + rng.uniform(-1.5, 0.5, n)], 1)
env = FpvVecEnv(p, num_envs=n, device=dev, object_list=world, per_drone_reset_pose=True, range_rays=rays.fan(9, 120.0, pitch_deg=15.0),
                range_max=RMAX)
state, rng_rows = env.batch.state, env.batch.range_rows
inv_poly = [float(c) for c in p.inverse_thrust_poly]
KV, KA, KW, G0 = 2.0, 8.0, 0.6, float(p.gravity)


def policy(see: bool):
    """fly +x at --speed and hold the height, by turning the thrust axis (body z) towards the wanted acceleration; with `see`,
    push away from whatever the fan reports closer than RMAX - sideways from the side rays, and to the side with more room (and
    back) from the three rays that look ahead"""
    q = state[6:10, :n]
    w, x, y, z = q[0], q[1], q[2], q[3]
    R0 = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y + w * z), 2 * (x * z - w * y)])      # the rows of R^T
    R1 = torch.stack([2 * (x * y - w * z), 1 - 2 * (x * x + z * z), 2 * (y * z + w * x)])
    up = torch.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)])
    v = state[3:6, :n]
    e = torch.stack([(a.speed - v[0]).clamp(-1.5, 1.5), -v[1], (2.0 * (Z0 - state[2, :n])).clamp(-2.0, 2.0) - v[2]])
    want = G0 * up + KV * torch.stack([(R0 * e).sum(0), (R1 * e).sum(0), (up * e).sum(0)])
    if see:
        close = (1.0 - rng_rows[:, :n] / RMAX).clamp_min(0.0)            # [9, n]: 0 = nothing within RMAX, 1 = touching
        left, ahead, right = close[0:3].amax(0), close[3:6].amax(0), close[6:9].amax(0)
        side = torch.where(left > right, -1.0, 1.0)                      # body +y is left: go where there is more room
        want[1] += KA * (right - left + side * ahead)
        want[0] -= KA * ahead
    norm = want.norm(dim=0).clamp_min(1e-3)
    thrust = (p.mass * want[2]).clamp(0.0, float(p.max_throttle_in_force))
    stick = torch.zeros_like(thrust)
    for c in inv_poly:                                                   # Horner: thrust [N] -> throttle percent
        stick = stick * thrust + c
    out = torch.stack([(-KW * want[1] / norm), (KW * want[0] / norm), torch.zeros_like(norm), (stick / 50.0 - 1.0)])
    return out.clamp(-1.0, 1.0)                                          # [4, n] SoA sticks, read in place


def fly(see: bool) -> int:
    env.reset(position=start)
    crashes = torch.zeros((), dtype=torch.int64, device=dev)
    for _ in range(a.steps):
        obs, reward, done, info = env.step(policy(see))
        crashes += done.sum()
    return int(crashes)


blind, seeing = fly(False), fly(True)
nearest = float(env.ranges.min())
print(f"{n} drones, {a.steps} steps of {p.dt * 1e3:.0f} ms at {a.speed} m/s through {len(world)} objects")
print(f"crashes without the sensor: {blind}")
print(f"crashes with the 9-ray fan:  {seeing}")
print(f"nearest range at the end: {nearest:.2f} m (max_range {RMAX} m)")
env.close()
