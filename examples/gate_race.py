#!/usr/bin/env python3
"""A drone race without a renderer: N drones fly a round course of gates, steered by a hand-written pursuit of `gate_obs` - the
next gate's centre and normal in the drone's body frame, which the step kernel writes next to the state.  The crossing test, the
race progress reward, the per-drone gate counter and the reset of a lane that finishes or crashes all happen inside the step
kernel (include/fpv_abi.h "Gate courses"); the loop below is policy + env.step and nothing else.

    python examples/gate_race.py --drones 4096 --steps 4000 --gates 8

Prints gates passed per second of wall-clock time, and how the race went.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fpyv_amd import gates, load_params  # noqa: E402
from fpyv_amd.env import FpvVecEnv  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--drones", type=int, default=4096)
ap.add_argument("--steps", type=int, default=4000)
ap.add_argument("--gates", type=int, default=8)
ap.add_argument("--radius", type=float, default=6.0)
ap.add_argument("--laps", type=int, default=1)
a = ap.parse_args()
dev = torch.device("cuda:0")
p = load_params(fps=1000, ceiling=100.0)
height = 10.0
track = gates.circular_track(a.gates, a.radius, 2.5, height=height)
n = a.drones
rng = np.random.default_rng(0)
# every drone starts one metre before "its" gate of the round course, with a little scatter, and restarts there
start = rng.integers(0, a.gates, n).astype(np.uint8)
rows = gates.derive(track).astype(np.float64)
pos = rows[start, 0:3] - 1.0 * rows[start, 3:6] + rng.uniform(-0.3, 0.3, (n, 3))
env = FpvVecEnv(p, num_envs=n, device=dev, gates=track, laps=a.laps, gate_start=start, per_drone_reset_pose=True)
env.reset(position=pos)
state, gobs = env.batch.state, env.batch.gate_obs_rows
inv_poly = [float(c) for c in p.inverse_thrust_poly]
KP, KD, KW, G0 = 6.0, 4.0, 0.6, float(p.gravity)


def policy():
    """thrust-vector pursuit: accelerate towards the gate centre (PD in the body frame) while holding the weight, by turning the
    thrust axis (body z) towards the wanted acceleration and pushing with its length"""
    q = state[6:10, :n]
    w, x, y, z = q[0], q[1], q[2], q[3]
    # R^T e_z (the world's up in the body frame) and R^T v
    up = torch.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)])
    v = state[3:6, :n]
    R0 = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y + w * z), 2 * (x * z - w * y)])
    R1 = torch.stack([2 * (x * y - w * z), 1 - 2 * (x * x + z * z), 2 * (y * z + w * x)])
    vb = torch.stack([(R0 * v).sum(0), (R1 * v).sum(0), (up * v).sum(0)])
    rel = gobs[0:3, :n] + 1.5 * gobs[3:6, :n]                   # aim a little behind the gate, along its normal
    want = G0 * up + KP * rel.clamp(-3.0, 3.0) - KD * vb
    norm = want.norm(dim=0).clamp_min(1e-3)
    thrust = (p.mass * want[2]).clamp(0.0, float(p.max_throttle_in_force))
    stick = torch.zeros_like(thrust)
    for c in inv_poly:                                           # Horner: thrust [N] -> throttle percent
        stick = stick * thrust + c
    out = torch.stack([(-KW * want[1] / norm), (KW * want[0] / norm), torch.zeros_like(norm), (stick / 50.0 - 1.0)])
    return out.clamp(-1.0, 1.0)                                  # [4, n] SoA sticks, read in place


passed = torch.zeros((), dtype=torch.int64, device=dev)
finished = torch.zeros((), dtype=torch.int64, device=dev)
crashed = torch.zeros((), dtype=torch.int64, device=dev)
ret = torch.zeros((), device=dev)
torch.cuda.synchronize()
t0 = time.perf_counter()
for t in range(a.steps):
    obs, reward, done, info = env.step(policy())
    ev = info["gate_event"]
    passed += ((ev == 1) | (ev == 3)).sum()
    finished += (ev == 3).sum()
    crashed += (done & (ev != 3)).sum()
    ret += reward.sum()
torch.cuda.synchronize()
dt = time.perf_counter() - t0
print(f"{n} drones, {a.steps} steps of 1 ms, {a.gates} gates on a circle of {a.radius} m, laps = {a.laps}: "
      f"{int(passed)} gates passed = {int(passed) / dt:,.0f} gates/s of wall-clock time ({n * a.steps / dt / 1e6:.1f} M env-steps/s), "
      f"{int(finished)} finishes, {int(crashed)} other resets, mean reward per step {float(ret) / (n * a.steps):+.4f}")
assert bool(torch.isfinite(state).all())
