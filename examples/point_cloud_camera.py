#!/usr/bin/env python3
"""The reference's simulator seen the reference's way, for N drones at once, headless: the world of src/core/simulator.py - a target
on a circular path, cylinders, gates, the ground - as POINT CLOUDS, splatted into every drone's FPV image by one kernel
(`Camera.render_depth_image`, components.py:614-629), and the chase of simulator.py:102-110 flown on the reference's own tracker, the
centroid of the lit pixels of a target-only render at max_depth 15:

    target_img = camera.render_depth_image([target], max_depth=15)                    -> chaser.render_points([target])
    target_pixels = mean(where(target_img > 0))[::-1]                                  -> chaser.points_centroid (NaN: not seen)
    rot_mat, force = drone.calculate_needed_force_orientation(target_pixels, target)   -> the same call, pixel = the centroid
    drone.step(action, ..., rotation_matrix=rot_mat, thrust_force=force)

The law is given the tracker's 64 x 48 camera (`set_chase_camera`): a centroid is in the pixels of the image it was taken from.
A drone that does not see the target has a NaN centroid, which the law takes as "not guided": it is left to its sticks
(simulator.py:104-105).  Every --every steps the full world is rendered too (max_depth 25, simulator.py:121) and at the end the images
of the first --save drones are written as .npy files.

    python examples/point_cloud_camera.py --drones 4096 --steps 600 --out /tmp/fpv_images
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
from fpyv_amd.clouds import PointCloud  # noqa: E402
from fpyv_amd.env import DroneBatch  # noqa: E402
from fpyv_amd.objects import Cylinder, Ground, Target  # noqa: E402
from fpyv_amd.splat import PointCloudCamera  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--drones", type=int, default=4096)
ap.add_argument("--steps", type=int, default=600)
ap.add_argument("--fps", type=float, default=250.0)
ap.add_argument("--every", type=int, default=10, help="render the full world every this many steps")
ap.add_argument("--save", type=int, default=4, help="drones whose last images are saved")
ap.add_argument("--out", default="point_cloud_images")
a = ap.parse_args()
dev, n = "cuda:0", a.drones
params = load_params(fps=a.fps)
target = Target(np.array([0.0, 0.0, 12.0]), 1.0, 3, {"radius": 25.0, "resolution": 20000})
world = [target, *gates.circular_track(6, 18.0, 2.5, height=6.0),
         *[Cylinder([12.0 * np.cos(k), 12.0 * np.sin(k), 0.0], 1.0, 8.0, 17, 17) for k in range(5)], Ground(80, 60)]
res = (64, 48)
chaser = DroneBatch(params, n, device=dev, cloud_camera=PointCloudCamera(resolution=res, max_depth=15.0, centroid=True))
rng = np.random.default_rng(0)
start = rng.uniform([13, -6, 7], [21, 6, 12], (n, 3)).astype(np.float32)           # behind the first point of the target's path
chaser.reset(position=start, velocity=np.zeros(3), ypr=np.zeros(3))
chaser.set_chase_camera(DepthCamera(resolution=res), max_depth=15.0)               # the law reads pixels of the tracker's 64 x 48 image
# the full view is a second camera: a second batch that is never stepped and is given the chaser's poses before it renders
viewer = DroneBatch(params, n, device=dev, cloud_camera=PointCloudCamera(resolution=res, max_depth=25.0))
viewer.reset()
cloud = PointCloud.from_world(world)              # flattened once; every render reads the target's position anew
sticks = torch.tensor([0.0, 0.0, 0.0, -0.646], device=dev).expand(n, 4).contiguous()
closest = torch.full((n,), float("inf"), device=dev)
tracked = torch.zeros((), dtype=torch.int64, device=dev)

torch.cuda.synchronize()
t0 = time.perf_counter()
for i in range(a.steps):
    target.update()                                                                # simulator.py:87
    chaser.render_points([target])                                                 # :102 - the offset moves, nothing is uploaded
    centroid = chaser.points_centroid                                              # :103-107
    tracked += (chaser.points_lit > 0).sum()
    rot_mat, force = chaser.calculate_needed_force_orientation(centroid, target)   # :109
    chaser.step(action=sticks, wind_velocity_vector=np.zeros(3), object_list=world, rotation_matrix=rot_mat, thrust_force=force,
                return_imu=False)                                                   # :110
    tpos = torch.as_tensor(np.asarray(target.position, dtype=np.float32), device=dev)
    closest = torch.minimum(closest, (tpos - chaser.position).norm(dim=1))
    if a.every and i % a.every == 0:
        viewer.state[:10].copy_(chaser.state[:10])
        viewer.render_points(cloud)                                                # :121
torch.cuda.synchronize()
dt = time.perf_counter() - t0
print(f"{n} drones x {a.steps} steps (dt = {params.dt * 1e3:.1f} ms) in {dt:.3f} s: a target-only render ({target.points.shape[0]} points), the "
      f"guidance law and a step per step, the full world ({cloud.total} points, {cloud.count} objects) every {a.every} steps")
print(f"tracked (a lit pixel): {int(tracked) / (n * a.steps):.2%} of the drone-steps; closest approach: median {float(closest.median()):.2f} m, "
      f"within 3 m: {int((closest < 3.0).sum())} of {n}; finite state: {bool(torch.isfinite(chaser.position).all())}")
os.makedirs(a.out, exist_ok=True)
k = min(a.save, n)
np.save(os.path.join(a.out, "world_u8.npy"), viewer.points_image[:k].cpu().numpy())
np.save(os.path.join(a.out, "target_u8.npy"), chaser.points_image[:k].cpu().numpy())
np.save(os.path.join(a.out, "centroid.npy"), chaser.points_centroid[:k].cpu().numpy())
print(f"saved world_u8.npy, target_u8.npy [{k}, {res[1]}, {res[0]}] and centroid.npy [{k}, 2] under {a.out}/; lit pixels of drone 0's world image: "
      f"{int((viewer.points_image[0] > 0).sum())}")
chaser.close()
