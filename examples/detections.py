#!/usr/bin/env python3
"""Object detections: N drones fly a round gate course between cylinders, and after every step one kernel gives each of them the 2-D
box of every object and gate in its FPV camera (the reference's 640 x 480, pitched 35 degrees, 120 degrees field of view), the depth
of its nearest in-front corner and whether the reference's pruning rule keeps it - `env.boxes`, `env.box_depth`, `env.box_visible`
(include/fpv_abi.h "Object detections").  The drones pursue their next gate on `gate_obs`; the visible boxes of drone 0 and the
detection rate are printed.

    python examples/detections.py --drones 4096 --steps 200
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fpyv_amd import gates, load_params  # noqa: E402
from fpyv_amd.detect import BoxDetector  # noqa: E402
from fpyv_amd.env import FpvVecEnv  # noqa: E402
from fpyv_amd.objects import Cylinder, Ground, Target  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--drones", type=int, default=4096)
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--gates", type=int, default=8)
ap.add_argument("--pixels", default="int", choices=["int", "float"])
ap.add_argument("--clip", action="store_true")
a = ap.parse_args()
dev = torch.device("cuda:0")
p = load_params(fps=200, ceiling=100.0)
n = a.drones
names = ["ground"] + [f"cylinder {k}" for k in range(6)] + ["target"]
world = [Ground(60, 4)] + [Cylinder([6.0 * np.cos(1.0 + k), 6.0 * np.sin(1.0 + k), 0.0], 0.5 + 0.1 * k, 3.0 + 0.5 * k) for k in range(6)]
world.append(Target([0.0, 0.0, 4.0], 0.8))
course = gates.circular_track(a.gates, 10.0, 2.5, height=3.0)
names += [f"gate {k} ({g.shape})" for k, g in enumerate(course)]
env = FpvVecEnv(p, num_envs=n, device=dev, object_list=world, gates=course, detector=BoxDetector(pixels=a.pixels, clip=a.clip),
                per_drone_reset_pose=True)
rng = np.random.default_rng(0)
th = rng.uniform(0.0, 2.0 * np.pi, n)
th[0] = 0.0
start = np.stack([10.0 * np.cos(th) + rng.uniform(-1, 1, n), 10.0 * np.sin(th) + rng.uniform(-1, 1, n), 3.0 + rng.uniform(-1, 1, n)], 1)
ypr = np.stack([np.zeros(n), np.zeros(n), np.rad2deg(th) + 90.0], 1)
env.reset(position=start, ypr=ypr)


def policy(gate_obs: torch.Tensor) -> torch.Tensor:
    """turn towards the next gate (its direction in the body frame) and hold a gentle forward pitch and throttle"""
    d = gate_obs[:, 0:3]
    yaw = torch.atan2(d[:, 1], d[:, 0]).clamp(-1.0, 1.0)
    climb = (0.2 * d[:, 2]).clamp(-0.3, 0.3)
    return torch.stack([torch.zeros_like(yaw), torch.full_like(yaw, 0.05), yaw, -0.25 + climb], 1)


for _ in range(5):                                   # the first calls load the kernels: not part of the rate
    env.step(policy(env.gate_obs))
torch.cuda.synchronize()
t0 = time.perf_counter()
seen = torch.zeros((), dtype=torch.int64, device=dev)
for _ in range(a.steps):
    obs, reward, done, info = env.step(policy(env.gate_obs))
    seen += info["box_visible"].sum()
torch.cuda.synchronize()
dt = time.perf_counter() - t0
boxes, depth, visible = env.boxes[:, :, 0].cpu().numpy(), env.box_depth[:, 0].cpu().numpy(), env.box_visible[:, 0].cpu().numpy()
m = boxes.shape[0]
print(f"{n} drones, {a.steps} steps of {p.dt * 1e3:.0f} ms, {len(world)} objects and {len(course)} gates = {m} boxes per drone, pixels {a.pixels}")
print("drone 0 sees:")
for k in range(m):
    if visible[k]:
        x0, y0, x1, y1 = boxes[k]
        print(f"  {names[k]:<24} ({x0:8.1f}, {y0:8.1f}) - ({x1:8.1f}, {y1:8.1f})   {depth[k]:6.2f} m")
print(f"  ({int(visible.sum())} of {m}; the others are behind it or off the image)")
print(f"visible boxes per drone and step: {int(seen) / (n * a.steps):.2f}")
print(f"{n * m * a.steps / dt:.3e} detections per second (steps, policy and detections together: {1e6 * dt / a.steps:.0f} us per step)")
env.close()
