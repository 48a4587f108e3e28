#!/usr/bin/env python3
"""Writes tests/golden/g23_splat.npz: captures of the reference's own splatted images - Camera.render_depth_image, render_image and
pruned_objects_list (src/utils/components.py:585-629) and the lit-pixel centroid of a target-only render as src/core/simulator.py:102-107
computes it - float64 / uint8, for tests/test_splat_host.py and tests/test_gpu_splat.py.

The reference is IMPORTED (oracle.gen_golden.import_reference: its pure-Python classes with the display modules stubbed) and run;
nothing of it is copied.  Needs the reference checkout oracle/gen_golden.py names; the committed .npz file is what the tests read.

Scene (every input rounded through float32): tools/gen_detect_golden.py's scene(seed 0) as the reference's own Ground(60, 40), three
Cylinder(..., angle_resolution=17, height_resolution=9), two Targets and six Gates (resolution 17) - 2225 points.  The stubbed
icosphere has one vertex, so the generator SUPPLIES the Targets' 42 unit vertices (fpyv_amd.clouds.icosphere(2), stored in the file)
and sets the reference's Target.vertices / current_vertices from them.  Object order: ground, cylinders, targets, gates.

Poses: POSES seeded draws of gen_detect_golden.draw_pose (seed 1) in its five kinds - looking at the scene, looking away, inverted,
inside a cylinder's box, close to a gate.  NO POSE IS SELECTED OR REDRAWN.  Two cameras, 64 x 48 and 16 x 12, fov 120, angle 35.

Per (camera, pose): render_depth_image(objects, max_depth=25), render_image(objects), per Target the target-only
render_depth_image([target], max_depth=15) with the centroid mean(where(img > 0))[::-1] and the count of lit pixels, the objects
pruned_objects_list keeps, and the reference's own projection_matrix.  Once: the reference's own `points` and `bbox3d` of every
object.  The tests form the float64 projection of every point from these - projection_matrix @ point is the reference's own formula
(:560) on the reference's own numbers.

Prints the measured guard bands (tests/splat_law.py measure): tol = 4 x the largest |fp32 host pixel coordinate - float64| and
tol_b = 4 x the largest |fp32 byte value - float64| over the in-image points, and what they leave out.
"""
import copy
import os
import sys

import numpy as np

REPO = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

OUT = os.path.join(REPO, "tests", "golden", "g23_splat.npz")
SCENE_SEED, POSE_SEED, POSES = 0, 1, 16
CAMERAS = [dict(resolution=[64, 48], fov=120.0, angle=35.0, rel=[0.1, 0.0, 0.0]),
           dict(resolution=[16, 12], fov=120.0, angle=35.0, rel=[0.1, 0.0, 0.0])]
GROUND_RES, ANGLE_RES, HEIGHT_RES, GATE_RES, NU = 40, 17, 9, 17, 2
MAX_DEPTH, TARGET_MAX_DEPTH = 25.0, 15.0


def capture():
    import gen_detect_golden as g
    from fpyv_amd.clouds import icosphere
    sc = g.scene(np.random.default_rng(SCENE_SEED))
    from oracle.gen_golden import import_reference
    import_reference()
    from utils.components import Camera, Cylinder, Gate, Ground, Target
    from utils.helper_functions import quaternion_to_rotation_matrix
    unit = g.f32(icosphere(NU))
    ground = Ground(int(sc["ground"]), GROUND_RES)
    cyls = [Cylinder(c["position"].copy(), c["radius"], c["height"], ANGLE_RES, HEIGHT_RES) for c in sc["cylinders"]]
    targets = []
    for s in sc["spheres"]:
        t = Target(s["position"].copy(), s["radius"], NU)
        t.vertices = unit * s["radius"]                       # (the stub gave one vertex: Target.__init__'s two lines, :759-760)
        t.current_vertices = t.vertices + t.position
        targets.append(t)
    gates = [Gate(x["position"].copy(), x["rotation"].copy(), x["size"], shape=x["shape"], resolution=GATE_RES) for x in sc["gates"]]
    objs = [ground, *cyls, *targets, *gates]
    M = len(objs)
    cams = [Camera(c["angle"], np.array(c["rel"]), list(c["resolution"]), fov=c["fov"]) for c in CAMERAS]
    rng = np.random.default_rng(POSE_SEED)
    P, Q, kinds = [], [], []
    for k in range(POSES):
        kind = g.KINDS[k % len(g.KINDS)]
        p, q = g.draw_pose(rng, kind, sc)
        P.append(p); Q.append(q); kinds.append(g.KINDS.index(kind))
    n, nc = POSES, len(cams)
    out = dict(proj=np.zeros((nc, n, 3, 4)), kept=np.zeros((nc, n, M), dtype=bool),
               target_centroid=np.full((nc, n, len(targets), 2), np.nan), target_lit=np.zeros((nc, n, len(targets)), dtype=np.int64))
    for c, cam in enumerate(cams):
        w, h = cam.resolution
        img = np.zeros((n, h, w), dtype=np.uint8); mask = np.zeros((n, h, w), dtype=np.uint8)
        timg = np.zeros((n, len(targets), h, w), dtype=np.uint8)
        for i in range(n):
            cam.update(P[i], quaternion_to_rotation_matrix(Q[i] / np.linalg.norm(Q[i])))
            out["proj"][c, i] = cam.projection_matrix
            survivors = cam.pruned_objects_list(copy.copy(objs))
            out["kept"][c, i] = [any(o is s for s in survivors) for o in objs]
            img[i] = cam.render_depth_image(copy.copy(objs), max_depth=MAX_DEPTH)
            if survivors:                                 # (render_image raises with every object pruned: the mask stays 0)
                mask[i] = cam.render_image(copy.copy(objs)).astype(np.uint8)
            for k, t in enumerate(targets):
                ti = cam.render_depth_image([t], max_depth=TARGET_MAX_DEPTH)
                timg[i, k] = ti
                px = np.array(np.where(ti > 0))                               # simulator.py:103-107
                out["target_lit"][c, i, k] = px.shape[1]
                if px.shape[1]:
                    out["target_centroid"][c, i, k] = px.mean(1)[::-1]
        out[f"image{c}"], out[f"mask{c}"], out[f"target_image{c}"] = img, mask, timg
    pts = [np.asarray(o.points, dtype=np.float64) for o in objs]
    gl = sc["gates"]
    shapes = ("rectangle", "circle", "half_circle")
    out.update(dict(
        p=np.array(P), q=np.array(Q), kind=np.array(kinds, dtype=np.int32),
        cam_resolution=np.array([c["resolution"] for c in CAMERAS], dtype=np.int32), cam_fov=np.array([c["fov"] for c in CAMERAS]),
        cam_angle=np.array([c["angle"] for c in CAMERAS]), cam_rel=np.array([c["rel"] for c in CAMERAS]),
        max_depth=np.float64(MAX_DEPTH), target_max_depth=np.float64(TARGET_MAX_DEPTH),
        ground_size=np.float64(sc["ground"]), ground_resolution=np.int32(GROUND_RES),
        cyl_position=np.array([c["position"] for c in sc["cylinders"]]), cyl_radius=np.array([c["radius"] for c in sc["cylinders"]]),
        cyl_height=np.array([c["height"] for c in sc["cylinders"]]), cyl_resolution=np.array([ANGLE_RES, HEIGHT_RES], dtype=np.int32),
        sph_position=np.array([s["position"] for s in sc["spheres"]]), sph_radius=np.array([s["radius"] for s in sc["spheres"]]),
        sph_vertices=unit,
        gate_position=np.array([x["position"] for x in gl]), gate_rotation=np.array([x["rotation"] for x in gl]),
        gate_size=np.array([x["size"] for x in gl]), gate_shape=np.array([shapes.index(x["shape"]) for x in gl], dtype=np.int32),
        gate_resolution=np.int32(GATE_RES),
        points=np.vstack(pts), first=np.concatenate([[0], np.cumsum([len(x) for x in pts])]).astype(np.int32),
        bbox3d=np.array([o.bbox3d for o in objs]),
        # object kind per slot: 0 ground, 1 cylinder, 2 target, 3 gate
        slot_kind=np.array([0] + [1] * len(cyls) + [2] * len(targets) + [3] * len(gates), dtype=np.int32)))
    return out


if __name__ == "__main__":
    cap = capture()
    np.savez_compressed(OUT, **cap)
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import splat_law
    splat_law._cache.clear()
    rep = splat_law.measure(cap)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes): {POSES} poses, no selection, {int(cap['first'][-1])} points, "
          f"poses per kind {np.bincount(cap['kind']).tolist()}")
    for k, v in rep.items():
        print(f"  {k}: {v}")
