"""The camera, the seeded scene and the float64 restatement that tests/test_depth_host.py (CPU) and tests/test_gpu_depth.py share
(include/fpv_abi.h "Depth camera").

The restatement is written from the definition, not from csrc/fpv_depth.h: the reference's camera formulas in float64 (focal
length, WORLD2CAM^T Rx(pitch), pixel centres through the inverse intrinsic matrix), fp32 poses and object rows widened to float64,
the textbook quadratic for ball and circle (tests/range_scene.py), one interval per convex solid, and a gate as the plate between
its aperture and the aperture grown by the frame width.
"""
import functools

import numpy as np

from fpyv_amd import gates as GT
from range_scene import Nearest, rot64, solids, table, world  # noqa: F401

MAX_DEPTH = 25.0
MARGIN = 1.0e-4             # range_scene's relative margins
EDGE = 1.0e-4               # a crossing point within this many metres of a frame edge is left out
WORLD2CAM = np.array([[0.0, 1.0, 0.0], [0.0, 0.0, -1.0], [1.0, 0.0, 0.0]])


def focal(width, fov_deg):
    return width / (2.0 * np.tan(np.deg2rad(fov_deg) / 2.0))


def rel_rot(pitch_deg):
    a = np.deg2rad(pitch_deg)
    rx = np.array([[1.0, 0.0, 0.0], [0.0, np.cos(a), -np.sin(a)], [0.0, np.sin(a), np.cos(a)]])
    return WORLD2CAM.T @ rx


def camera_pose(p, q, pitch_deg, rel_pos):
    """(o [n, 3], C [n, 3, 3]) float64: origin p + R(q) rel_pos and camera rotation R(q) rel_rot"""
    R = rot64(q)
    return p.astype(np.float64) + R @ np.asarray(rel_pos, dtype=np.float64), R @ rel_rot(pitch_deg)


def pixel_dirs_cam(width, height, fov_deg):
    """[H, W, 3] camera-frame directions K^-1 (i + 1/2, j + 1/2, 1) of the pixel centres: z = 1"""
    f = focal(width, fov_deg)
    K = np.array([[f, 0.0, width / 2], [0.0, f, height / 2], [0.0, 0.0, 1.0]])
    j, i = np.meshgrid(np.arange(height) + 0.5, np.arange(width) + 0.5, indexing="ij")
    return np.stack([i, j, np.ones_like(i)], -1) @ np.linalg.inv(K).T


def course(count, radius=6.5, size=2.4, height=3.0):
    """`count` gates of all three shapes around the scene, every third one pitched out of the vertical"""
    out = GT.circular_track(count, radius, size, height=height)
    for k, g in enumerate(out):
        if k % 3 == 2:
            a = 0.35 + 0.01 * k
            tilt = np.array([[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]])
            out[k] = type(g)(g.position + np.array([0.0, 0.0, 0.3 * (k % 5)]), g.rotation_matrix @ tilt, g.size, shape=g.shape)
    return out


@functools.lru_cache(maxsize=None)
def scene(n=256, seed=19):
    """(p [n, 3], q [n, 4] wxyz) float32: p uniform in [-8, 8]^2 x [0.3, 7], q a flying attitude - any yaw, up to ~35 degrees of
    roll and pitch.  Computed once; treat as read-only."""
    rng = np.random.default_rng(seed)
    p = np.stack([rng.uniform(-8, 8, n), rng.uniform(-8, 8, n), rng.uniform(0.3, 7, n)], 1).astype(np.float32)
    yaw, tilt, axis = rng.uniform(-np.pi, np.pi, n), rng.uniform(0.0, 0.6, n), rng.uniform(-np.pi, np.pi, n)
    qz = np.stack([np.cos(yaw / 2), 0 * yaw, 0 * yaw, np.sin(yaw / 2)], 1)
    qt = np.stack([np.cos(tilt / 2), np.sin(tilt / 2) * np.cos(axis), np.sin(tilt / 2) * np.sin(axis), 0 * tilt], 1)
    w1, x1, y1, z1 = qz.T
    w2, x2, y2, z2 = qt.T
    q = np.stack([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                  w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2], 1)
    return p, (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)


def cast(o, d, object_list=(), gate_rows=None, frame=0.15, max_depth=MAX_DEPTH):
    """float64, from the definition, for origins o [n, 3] and directions d [n, ..., 3] (any shape between).  Returns (depth, nearest
    thing: object index, 100 + gate index, or -1, keep, scale): `keep` is False where a margin of the restatement is too small
    to call (range_scene's, plus a crossing point within EDGE of a frame edge); `scale` is max(depth, distance from the origin to
    the nearest thing's centre) - what an error is measured in."""
    near = Nearest(o, d)
    oo, shape = near.oo, near.shape
    solids(near, d, object_list)
    if gate_rows is not None:
        for g, row in enumerate(np.asarray(gate_rows, dtype=np.float32).astype(np.float64)):
            c, nrm, u, w = row[0:3], row[3:6], row[6:9], row[9:12]
            a, hz, zc, r2 = row[12:16]
            nd, s = d @ nrm, (oo - c) @ nrm
            par = np.abs(nd) < 1e-12
            with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
                t = np.where(par, np.inf, -s / np.where(par, 1.0, nd))
                x = (oo - c) + t[..., None] * d
                y, z = x @ u, x @ w
                rho = np.sqrt(y * y + (z - zc) ** 2)
                rin, rout = np.sqrt(r2), np.sqrt(r2) + frame
                outer = (np.abs(y) <= a + frame) & (np.abs(z) <= hz + frame) & (rho <= rout)
                inner = (np.abs(y) <= a) & (np.abs(z) <= hz) & (rho <= rin)
                edge = np.minimum.reduce([np.abs(np.abs(y) - a), np.abs(np.abs(y) - a - frame), np.abs(np.abs(z) - hz),
                                          np.abs(np.abs(z) - hz - frame),
                                          np.abs(rho - rin) if np.isfinite(rin) else np.full(shape, np.inf),
                                          np.abs(rho - rout) if np.isfinite(rout) else np.full(shape, np.inf)])
            front = ~par & (t >= 0) & np.isfinite(t)
            ok = ~front | (edge >= EDGE) | (t > 2 * max_depth)
            near.take(t, front & outer & ~inner, ok, 100 + g, c)
    return near.result(max_depth) + ((near.pairs, near.dropped),)


def restate(p, q, cam, object_list=(), gate_rows=None):
    """The images of `cam` (a fpyv_amd.camera.DepthCamera; only its constructor arguments are read) for drones at p, q, in
    float64: (depth [n, H, W] metres, nearest, keep, scale, (pairs, dropped))."""
    o, C = camera_pose(p, q, cam.camera_angle, cam.relative_position)
    d = np.einsum("nab,hwb->nhwa", C, pixel_dirs_cam(cam.resolution[0], cam.resolution[1], cam.fov))
    return cast(o, d, object_list, gate_rows, cam.gate_frame, cam.max_depth)
