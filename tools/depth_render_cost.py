#!/usr/bin/env python3
"""What a depth render costs: in ONE process on one MI355X, HIP-event-timed chains of launches - the render of 32 x 24
and 64 x 48 images, metres and bytes, against the ground only, the four-object G10 world, eight objects and the G10 world plus a
course of 12 gates, and as the yardstick the range scan of 32 rays on the same drones and worlds - interleaved over several
rounds, at 4096 and 65536 drones.  Writes profiles/depth_render.md: per leg the time per launch, per image, and per pixel (ray)
and thing.

    python tools/depth_render_cost.py [--n 4096 65536] [--launches 100] [--rounds 5] [--out profiles/depth_render.md]

The drones are scattered over [-8, 8]^2 x [0.5, 7] m at flying attitudes (the scene of tests/depth_scene.py, larger).  No threshold
is asserted: the feature has no predecessor to compare with.
"""
import argparse
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from fpyv_amd import gates, load_params, rays  # noqa: E402
from fpyv_amd.camera import DepthCamera  # noqa: E402
from fpyv_amd.env import DroneBatch  # noqa: E402
from fpyv_amd.objects import Cylinder, Ground, Target  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, nargs="*", default=[4096, 65536])
ap.add_argument("--launches", type=int, default=100)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "depth_render.md"))
a = ap.parse_args()
dev = torch.device("cuda:0")
p = load_params(fps=1000, ceiling=100.0)
TABLE = [Target([1.5, -6.0, 3.0], 0.8), Cylinder([3.0, 0.0, 0.0], 1.0, 5.0), Cylinder([-2.0, 2.5, 0.0], 0.6, 1.5), Ground(),
         Target([-5.0, -5.0, 2.0], 1.5), Cylinder([6.0, 6.0, 0.0], 0.5, 7.0), Target([0.0, 4.0, 6.0], 1.0), Cylinder([-6.0, 3.0, 1.0], 2.0, 2.0)]
COURSE = gates.circular_track(12, 6.5, 2.4, height=3.0)
WORLDS = {"ground only": ([TABLE[3]], 0), "G10 world": (TABLE[:4], 0), "8 objects": (TABLE, 0), "G10 world + 12 gates": (TABLE[:4], 12)}
DMAX, RAYS = 25.0, 32
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
lines = ["# What a depth render costs (DESIGN 3.8)", "",
         f"One MI355X, one process, `tools/depth_render_cost.py`: HIP-event chains of {a.launches} launches, {a.rounds} rounds interleaved, median;",
         "drones scattered over [-8, 8]^2 x [0.5, 7] m at flying attitudes, the reference's camera (35 degrees, fov 120), max_depth 25 m;",
         f"the yardstick is the range scan of {RAYS} random unit rays (max_range 25 m) on the same drones and objects.", ""]


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
    rng = np.random.default_rng(19)
    pos = np.stack([rng.uniform(-8, 8, n), rng.uniform(-8, 8, n), rng.uniform(0.5, 7, n)], 1).astype(np.float32)
    ypr = (rng.uniform(-180, 180, (n, 3)) * np.array([0.2, 0.2, 1.0])).astype(np.float32)
    kw = dict(device=dev, auto_reset=True, with_accel=False)
    ray_set = rays.derive(np.random.default_rng(3).normal(size=(RAYS, 3)))
    legs = {}
    keep = []
    for res in ((32, 24), (64, 48)):
        for enc in ("metres", "u8"):
            cam = DepthCamera(resolution=res, max_depth=DMAX, encoding=enc)
            plain, gated = DroneBatch(p, n, depth_camera=cam, **kw), DroneBatch(p, n, depth_camera=cam, gates=COURSE, **kw)
            keep += [plain, gated]
            for b in (plain, gated):
                b.reset(position=pos, ypr=ypr)
            for wname, (world, ng) in WORLDS.items():
                if enc == "u8" and wname != "G10 world":
                    continue
                legs[f"{res[0]} x {res[1]} {enc}, {wname}"] = (lambda b=(gated if ng else plain), w=world: b.render_depth(w), res[0] * res[1], len(world) + ng)
    scan = DroneBatch(p, n, range_rays=ray_set, range_max=DMAX, **kw)
    scan.reset(position=pos, ypr=ypr)
    for wname, (world, ng) in WORLDS.items():
        if not ng:
            legs[f"range scan, {RAYS} rays, {wname}"] = (lambda b=scan, w=world: b.range_scan(w), RAYS, len(world))
    res_t = {k: [] for k in legs}
    for r in range(a.rounds + 1):
        for name, (fn, px, k) in legs.items():
            t = timed(fn, a.launches)
            if r:
                res_t[name].append(t)
    lines += [f"## {n} drones", "", "| leg | us / launch | min | ns / image (drone) | ps / (pixel or ray, thing) |", "|---|---:|---:|---:|---:|"]
    for name, (fn, px, k) in legs.items():
        med = statistics.median(res_t[name])
        lines.append(f"| {name} | {med:.2f} | {min(res_t[name]):.2f} | {med * 1e3 / n:.2f} | {med * 1e6 / (n * px * k):.3f} |")
    lines.append("")
    print("\n".join(lines[-(len(legs) + 5):]), flush=True)
    del keep, scan, legs
    torch.cuda.empty_cache()
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w", encoding="utf-8") as f:
    f.write("\n".join(lines) + "\n")
