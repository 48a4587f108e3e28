#!/usr/bin/env python3
"""What a range scan costs: in ONE process on one MI355X, HIP-event-timed chains of launches - the scan alone for
8 / 16 / 32 rays against the ground only, the four-object G10 world and eight objects, and the loop `step; scan` (16 rays, G10
world) against `step` alone - interleaved over several rounds, at 2^20 and 2^23 drones.  Writes profiles/range_scan.md: per leg
the time, the bandwidth on the scan's own 28 + 4 R bytes per drone, and the scan's time per drone, ray and object.

    python tools/range_scan_cost.py [--n 1048576 8388608] [--launches 1000] [--rounds 5] [--out profiles/range_scan.md]

The drones are scattered over [-8, 8]^2 x [0.5, 8] m at random attitudes (the scene of tests/range_scene.py, larger): about 45 %
of the rays hit something, and the wave-level cull finds every object near some lane of almost every wave - the scan's expensive
case.  No threshold is asserted: the feature has no predecessor to compare with.
"""
import argparse
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from fpyv_amd import load_params, rays, sticks  # noqa: E402
from fpyv_amd.env import DroneBatch  # noqa: E402
from fpyv_amd.objects import Cylinder, Ground, Target  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, nargs="*", default=[1 << 20, 1 << 23])
ap.add_argument("--launches", type=int, default=1000)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "range_scan.md"))
a = ap.parse_args()
dev = torch.device("cuda:0")
p = load_params(fps=1000, ceiling=100.0)
TABLE = [Target([1.5, -6.0, 3.0], 0.8), Cylinder([3.0, 0.0, 0.0], 1.0, 5.0), Cylinder([-2.0, 2.5, 0.0], 0.6, 1.5), Ground(),
         Target([-5.0, -5.0, 2.0], 1.5), Cylinder([6.0, 6.0, 0.0], 0.5, 7.0), Target([0.0, 4.0, 6.0], 1.0), Cylinder([-6.0, 3.0, 1.0], 2.0, 2.0)]
WORLDS = {"ground only": [TABLE[3]], "G10 world": TABLE[:4], "8 objects": TABLE}
RMAX = 20.0
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
lines = ["# What a range scan costs (DESIGN 3.7)", "",
         f"One MI355X, one process, `tools/range_scan_cost.py`: HIP-event chains of {a.launches} launches, {a.rounds} rounds interleaved, median;",
         "drones scattered over [-8, 8]^2 x [0.5, 8] m at random attitudes, random unit rays, max_range 20 m.", ""]


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


for n in a.n:
    g = torch.Generator().manual_seed(3)
    ray_sets = {R: rays.derive(torch.randn((R, 3), generator=g, dtype=torch.float64).numpy()) for R in (8, 16, 32)}
    rng = np.random.default_rng(11)
    pos = np.stack([rng.uniform(-8, 8, n), rng.uniform(-8, 8, n), rng.uniform(0.5, 8, n)], 1).astype(np.float32)
    ypr = rng.uniform(-180, 180, (n, 3)).astype(np.float32)
    kw = dict(device=dev, auto_reset=True, with_accel=False)
    scat = {R: DroneBatch(p, n, range_rays=ray_sets[R], range_max=RMAX, **kw) for R in (8, 16, 32)}
    for b in scat.values():
        b.reset(position=pos, ypr=ypr)
    ring = 32 if n <= (1 << 21) else 4
    acts = sticks.ema_noise_device(ring, n, dev)
    plain = DroneBatch(p, n, **kw)
    both = DroneBatch(p, n, range_rays=ray_sets[16], range_max=RMAX, **kw)
    legs = {}
    for R in (8, 16, 32):
        for wname, world in WORLDS.items():
            legs[f"scan, {R} rays, {wname}"] = (lambda b=scat[R], w=world: b.range_scan(w), R, len(world))

    def step_only(b=plain):
        for t in range(ring):
            b._step_raw(acts[t])

    def step_scan(b=both, w=WORLDS["G10 world"]):
        for t in range(ring):
            b._step_raw(acts[t])
            b.range_scan(w)

    res = {k: [] for k in list(legs) + ["step", "step; scan"]}
    reps_loop = max(1, a.launches // ring)
    for r in range(a.rounds + 1):
        for name, (fn, R, k) in legs.items():
            t = timed(fn, a.launches)
            if r:
                res[name].append(t)
        for name, fn, b in (("step", step_only, plain), ("step; scan", step_scan, both)):
            b.reset(position=pos, ypr=ypr)
            t = timed(fn, reps_loop) / ring
            if r:
                res[name].append(t)
    lines += [f"## {n} drones", "", "| scan alone | us / scan | min | bytes / drone | GB/s on its own bytes | of 8 TB/s | ps / (drone ray object) |",
              "|---|---:|---:|---:|---:|---:|---:|"]
    for name, (fn, R, k) in legs.items():
        med, nbytes = statistics.median(res[name]), 28 + 4 * R
        lines.append(f"| {name} | {med:.2f} | {min(res[name]):.2f} | {nbytes} | {nbytes * n / med / 1e3:.0f} | {nbytes * n / med / 1e3 / 8000:.1%} | "
                     f"{med * 1e6 / (n * R * k):.2f} |")
    s, ss = statistics.median(res["step"]), statistics.median(res["step; scan"])
    lines += ["", "| loop, us per env-step | median | min |", "|---|---:|---:|", f"| `step` (headline kernel, 133 B) | {s:.2f} | {min(res['step']):.2f} |",
              f"| `step; scan` (16 rays, G10 world) | {ss:.2f} | {min(res['step; scan']):.2f} |",
              f"| the scan inside the loop | {ss - s:.2f} | - |", ""]
    print("\n".join(lines[-(len(legs) + 12):]), flush=True)
    del scat, plain, both, legs
    torch.cuda.empty_cache()
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w", encoding="utf-8") as f:
    f.write("\n".join(lines) + "\n")
