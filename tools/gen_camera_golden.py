"""tests/golden/g19_camera.npz: the reference's own Camera geometry and point clouds for tests/test_depth_host.py - data only.

For the reference's Camera(35.0, [0.1, 0, 0], [64, 48], fov=120.0) and six seeded drone poses (1-6 m above the ground, any yaw,
moderate roll and pitch): focal_length, intrinsic_matrix, relative_rotation_matrix; per pose the camera's position and
rotation_matrix after update(), its projection_matrix, and pixel2direction at a sample of real-valued pixels in the 'drone' and
'world' frames.  The world is a Ground(60, 50, random=False) and three non-random Cylinders, each taller than the highest pose (the
reference's cloud has no cap; the solid here has one): their `points` and constructor arguments.
Runs where the reference is checked out (oracle.gen_golden.import_reference); the fixture is committed, this script only documents
how it was made:  python tools/gen_camera_golden.py
"""
import os
import sys

import numpy as np

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, REPO)

CAMERA = dict(camera_pitch_angle=35.0, position_relative_to_frame=[0.1, 0.0, 0.0], resolution=[64, 48], fov=120.0)
GROUND = dict(size=60, resolution=50)
# (radii and positions that fp32 holds exactly: the object rows are fp32)
CYLINDERS = [dict(position=[6.0, 2.0, 0.0], radius=1.0, height=8.0, angle_resolution=40, height_resolution=30),
             dict(position=[-5.0, -6.0, 0.0], radius=0.75, height=7.0, angle_resolution=32, height_resolution=20),
             dict(position=[0.5, 8.0, 0.0], radius=1.5, height=7.5, angle_resolution=32, height_resolution=18)]
POSES = 6
PIXELS = 24


def main():
    from oracle import gen_golden
    gen_golden.import_reference()
    from utils.components import Camera, Cylinder, Ground
    from utils.helper_functions import euler_angles_to_rotation_matrix
    rng = np.random.default_rng(19)
    cam = Camera(CAMERA["camera_pitch_angle"], np.array(CAMERA["position_relative_to_frame"]), CAMERA["resolution"], fov=CAMERA["fov"])
    pos = np.stack([rng.uniform(-4.0, 4.0, POSES), rng.uniform(-4.0, 4.0, POSES), np.linspace(1.0, 6.0, POSES)], 1)
    rpy = np.stack([rng.uniform(-0.4, 0.4, POSES), rng.uniform(-0.4, 0.4, POSES), rng.uniform(-np.pi, np.pi, POSES)], 1)
    rot = np.array([euler_angles_to_rotation_matrix(*a) for a in rpy])
    pixels = np.stack([rng.uniform(0.0, 64.0, PIXELS), rng.uniform(0.0, 48.0, PIXELS)], 1)
    cam_pos, cam_rot, proj, dir_drone, dir_world = [], [], [], [], []
    for p, R in zip(pos, rot):
        cam.update(p, R)
        cam_pos.append(np.array(cam.position)); cam_rot.append(np.array(cam.rotation_matrix)); proj.append(np.array(cam.projection_matrix))
        dir_drone.append([cam.pixel2direction(px, ref_frame="drone") for px in pixels])
        dir_world.append([cam.pixel2direction(px, ref_frame="world") for px in pixels])
    ground = Ground(GROUND["size"], GROUND["resolution"], random=False)
    cyls = [Cylinder(np.array(c["position"]), c["radius"], c["height"], c["angle_resolution"], c["height_resolution"], random=False)
            for c in CYLINDERS]
    f64 = lambda a: np.asarray(a, dtype=np.float64)  # noqa: E731
    out = {"camera_pitch_angle": f64(CAMERA["camera_pitch_angle"]), "position_relative_to_frame": f64(CAMERA["position_relative_to_frame"]),
           "resolution": np.array(CAMERA["resolution"], dtype=np.int64), "fov": f64(CAMERA["fov"]),
           "focal_length": f64(cam.focal_length), "intrinsic_matrix": f64(cam.intrinsic_matrix),
           "relative_rotation_matrix": f64(cam.relative_rotation_matrix),
           "drone_position": pos, "drone_rotation_matrix": rot, "position": f64(cam_pos), "rotation_matrix": f64(cam_rot),
           "projection_matrix": f64(proj), "pixels": pixels, "direction_drone": f64(dir_drone), "direction_world": f64(dir_world),
           "ground_args": f64([GROUND["size"], GROUND["resolution"]]), "ground_points": f64(ground.points),
           "cylinder_args": f64([c["position"] + [c["radius"], c["height"], c["angle_resolution"], c["height_resolution"]] for c in CYLINDERS])}
    for k, c in enumerate(cyls):
        out[f"cylinder{k}_points"] = f64(c.points)
    path = os.path.join(REPO, "tests", "golden", "g19_camera.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
