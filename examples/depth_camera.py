#!/usr/bin/env python3
"""First-person depth images: N drones fly a round gate course over a world of two cylinders, a sphere and the ground, each with
the reference's FPV camera (pitched 35 degrees, 120 degrees field of view) - `env.depth`, which a render kernel writes after every
step (include/fpv_abi.h "Depth camera").  The drones pursue their next gate on `gate_obs`; a few of the last images are written as
.npy files and the render rate is printed.

    python examples/depth_camera.py --drones 4096 --steps 400 --out /tmp/depth
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fpyv_amd import gates, load_params  # noqa: E402
from fpyv_amd.camera import DepthCamera  # noqa: E402
from fpyv_amd.env import FpvVecEnv  # noqa: E402
from fpyv_amd.objects import Cylinder, Ground, Target  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--drones", type=int, default=4096)
ap.add_argument("--steps", type=int, default=400)
ap.add_argument("--images", type=int, default=4)
ap.add_argument("--encoding", default="metres", choices=["metres", "u8"])
ap.add_argument("--out", default=".")
a = ap.parse_args()
dev = torch.device("cuda:0")
p = load_params(fps=200, ceiling=100.0)
n = a.drones
world = [Target([1.5, -6.0, 3.0], 0.8), Cylinder([3.0, 0.0, 0.0], 1.0, 5.0), Cylinder([-2.0, 2.5, 0.0], 0.6, 1.5), Ground()]
course = gates.circular_track(12, 10.0, 2.5, height=3.0)
cam = DepthCamera(resolution=(64, 48), max_depth=25.0, encoding=a.encoding)
env = FpvVecEnv(p, num_envs=n, device=dev, object_list=world, gates=course, depth_camera=cam, per_drone_reset_pose=True)
rng = np.random.default_rng(0)
th = rng.uniform(0.0, 2.0 * np.pi, n)
start = np.stack([10.0 * np.cos(th) + rng.uniform(-1, 1, n), 10.0 * np.sin(th) + rng.uniform(-1, 1, n), 3.0 + rng.uniform(-1, 1, n)], 1)
ypr = np.stack([np.zeros(n), np.zeros(n), np.rad2deg(th) + 90.0], 1)
env.reset(position=start, ypr=ypr)


def policy(gate_obs: torch.Tensor) -> torch.Tensor:
    """turn towards the next gate (its direction in the body frame) and hold a gentle forward pitch and throttle"""
    d = gate_obs[:, 0:3]
    yaw = torch.atan2(d[:, 1], d[:, 0]).clamp(-1.0, 1.0)
    climb = (0.2 * d[:, 2]).clamp(-0.3, 0.3)
    return torch.stack([torch.zeros_like(yaw), torch.full_like(yaw, 0.05), yaw, -0.25 + climb], 1)


torch.cuda.synchronize()
t0 = time.perf_counter()
passed = torch.zeros((), dtype=torch.int64, device=dev)
for _ in range(a.steps):
    obs, reward, done, info = env.step(policy(env.gate_obs))
    passed += (info["gate_event"] == 1).sum()
torch.cuda.synchronize()
dt = time.perf_counter() - t0
depth = env.depth
os.makedirs(a.out, exist_ok=True)
for k in range(min(a.images, n)):
    np.save(os.path.join(a.out, f"depth_{k}.npy"), depth[k].cpu().numpy())
pixels = n * cam.resolution[0] * cam.resolution[1] * a.steps
seen = float((depth.float() != (0.0 if a.encoding == "u8" else cam.max_depth)).float().mean())
print(f"{n} drones, {a.steps} steps of {p.dt * 1e3:.0f} ms, {len(world)} objects and {len(course)} gates, {cam.resolution[0]} x {cam.resolution[1]} {a.encoding} images")
print(f"gates passed: {int(passed)}; pixels that see something in the last images: {100 * seen:.1f} %")
print(f"{pixels / dt:.3e} pixels per second (steps, policy and renders together: {1e6 * dt / a.steps:.0f} us per step)")
print(f"wrote {min(a.images, n)} images to {os.path.abspath(a.out)}")
env.close()
