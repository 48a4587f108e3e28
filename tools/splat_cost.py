#!/usr/bin/env python3
"""What a point-cloud render costs: in ONE process on one MI355X, HIP-event-timed chains of launches - the splat of
32 x 24 and 64 x 48 byte images over a world of about 2 k and one of about 20 k points, with and without the centroid, and as the
yardstick the analytic depth render of the same image size over the same ground, cylinders and target - interleaved over
several rounds, at 4096 and 65536 drones.  Writes profiles/splat_render.md: per leg the time per launch, per image, and per point.

    python tools/splat_cost.py [--n 4096 65536] [--launches 50] [--rounds 5] [--out profiles/splat_render.md]

The drones are scattered over [-8, 8]^2 x [0.5, 7] m at flying attitudes (the scene of tools/depth_render_cost.py).  One workgroup
renders one drone: every workgroup reads the whole cloud, 12 P bytes for P points, which the L2 serves after the first.  No threshold
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

from fpyv_amd import load_params  # noqa: E402
from fpyv_amd.camera import DepthCamera  # noqa: E402
from fpyv_amd.clouds import PointCloud  # noqa: E402
from fpyv_amd.env import DroneBatch  # noqa: E402
from fpyv_amd.objects import Cylinder, Ground, Target  # noqa: E402
from fpyv_amd.splat import PointCloudCamera  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, nargs="*", default=[4096, 65536])
ap.add_argument("--launches", type=int, default=50)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "splat_render.md"))
a = ap.parse_args()
dev = torch.device("cuda:0")
p = load_params(fps=1000, ceiling=100.0)


def world(ground_res, angle_res, height_res, nu):
    return [Ground(40, ground_res), Cylinder([3.0, 0.0, 0.0], 1.0, 5.0, angle_res, height_res), Cylinder([-2.0, 2.5, 0.0], 0.6, 1.5, angle_res, height_res),
            Cylinder([6.0, 6.0, 0.0], 0.5, 7.0, angle_res, height_res), Target([1.5, -6.0, 3.0], 0.8, nu)]


WORLDS = {"2 k": world(40, 17, 9, 2), "20 k": world(130, 33, 30, 5)}
CLOUDS = {k: PointCloud.from_world(w) for k, w in WORLDS.items()}
DMAX = 25.0
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
lines = ["# What a point-cloud render costs (DESIGN 3.13)", "",
         f"One MI355X, one process, `tools/splat_cost.py`: HIP-event chains of {a.launches} launches, {a.rounds} rounds interleaved, median;",
         "drones scattered over [-8, 8]^2 x [0.5, 7] m at flying attitudes, the reference's camera (35 degrees, fov 120), max_depth 25 m, byte images;",
         "worlds: a ground grid, three cylinders and a target of " + " and ".join(f"{c.total} points" for c in CLOUDS.values()) + ";",
         "the yardstick is the analytic depth render (DESIGN 3.8) of the same image size over the same five solids.", ""]


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
    legs, keep = {}, []
    for res in ((32, 24), (64, 48)):
        for cen in (False, True):
            b = DroneBatch(p, n, cloud_camera=PointCloudCamera(resolution=res, max_depth=DMAX, centroid=cen), **kw)
            b.reset(position=pos, ypr=ypr)
            keep.append(b)
            for wname, cl in CLOUDS.items():
                if cen and wname != "2 k":
                    continue
                legs[f"splat {res[0]} x {res[1]}, {wname} points{', centroid' if cen else ''}"] = (lambda b=b, c=cl: b.render_points(c), cl.total)
        d = DroneBatch(p, n, depth_camera=DepthCamera(resolution=res, max_depth=DMAX, encoding="u8"), **kw)
        d.reset(position=pos, ypr=ypr)
        keep.append(d)
        legs[f"analytic depth render {res[0]} x {res[1]}, 5 solids"] = (lambda b=d, w=WORLDS["2 k"]: b.render_depth(w), 0)
    res_t = {k: [] for k in legs}
    for r in range(a.rounds + 1):
        for name, (fn, pts) in legs.items():
            t = timed(fn, a.launches)
            if r:
                res_t[name].append(t)
    lines += [f"## {n} drones", "", "| leg | us / launch | min | ns / image (drone) | ps / (drone, point) |", "|---|---:|---:|---:|---:|"]
    for name, (fn, pts) in legs.items():
        med = statistics.median(res_t[name])
        per = f"{med * 1e6 / (n * pts):.3f}" if pts else "-"
        lines.append(f"| {name} | {med:.2f} | {min(res_t[name]):.2f} | {med * 1e3 / n:.2f} | {per} |")
    lines.append("")
    print("\n".join(lines[-(len(legs) + 5):]), flush=True)
    del keep, legs
    torch.cuda.empty_cache()
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w", encoding="utf-8") as f:
    f.write("\n".join(lines) + "\n")
