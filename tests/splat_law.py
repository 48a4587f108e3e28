"""What the point-cloud camera's tests share: the g23 capture of the reference's splatted images (tools/gen_splat_golden.py), the
scene and the cameras it describes as this package's objects, the float64 projection of every captured point through the reference's
own captured projection matrices, the fragile pixels that projection alone marks, and the comparison of a rendered image with the
capture (tests/test_splat_host.py on the host function, tests/test_gpu_splat.py on the kernel).  Nothing here is used by the product."""
import os

import numpy as np

import detect_law

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g23_splat.npz")
# 4 x the largest |fp32 host value - float64 value| over the in-image points of the g23 capture (measure() below):
TOL = 1.72e-4         # pixels: measured 1.7162e-4 (largest error 4.29e-5 pixels)
TOL_B = 2.62e-4       # byte levels: measured 2.6186e-4 (largest error 6.55e-5 levels)
SHAPES = ("rectangle", "circle", "half_circle")
_cache = {}


def load():
    if "cap" not in _cache:
        with np.load(GOLDEN) as z:
            _cache["cap"] = {k: z[k] for k in z.files}
    return _cache["cap"]


def scene(cap):
    """the object list of the capture as this package's objects: ground, cylinders, targets (the captured unit vertices), gates"""
    from fpyv_amd.objects import Cylinder, Gate, Ground, Target
    ar, hr = (int(x) for x in cap["cyl_resolution"])
    objs = [Ground(float(cap["ground_size"]), int(cap["ground_resolution"]))]
    objs += [Cylinder(p, float(r), float(h), ar, hr) for p, r, h in zip(cap["cyl_position"], cap["cyl_radius"], cap["cyl_height"])]
    objs += [Target(p, float(r), vertices=cap["sph_vertices"]) for p, r in zip(cap["sph_position"], cap["sph_radius"])]
    objs += [Gate(p, R, float(s), shape=SHAPES[int(k)], resolution=int(cap["gate_resolution"]))
             for p, R, s, k in zip(cap["gate_position"], cap["gate_rotation"], cap["gate_size"], cap["gate_shape"])]
    return objs


def camera(cap, c, **kw):
    from fpyv_amd.splat import PointCloudCamera
    kw.setdefault("max_depth", float(cap["max_depth"]))
    return PointCloudCamera(resolution=[int(x) for x in cap["cam_resolution"][c]], fov=float(cap["cam_fov"][c]),
                            camera_angle=float(cap["cam_angle"][c]), position_relative_to_frame=cap["cam_rel"][c], **kw)


def cloud(cap):
    if "cloud" not in _cache:
        from fpyv_amd.clouds import PointCloud
        _cache["cloud"] = PointCloud.from_world(scene(cap))
    return _cache["cloud"]


def project64(cap, c, points=None):
    """(u [n, P], v [n, P], z [n, P]) float64, untruncated: the reference's projection_matrix @ (X, 1), divided by the depth (:560-566)"""
    X = cap["points"] if points is None else points
    h = np.vstack([X.T, np.ones(X.shape[0])])
    r = np.einsum("nab,bp->nap", cap["proj"][c], h)
    with np.errstate(divide="ignore", invalid="ignore"):
        return r[:, 0] / r[:, 2], r[:, 1] / r[:, 2], r[:, 2]


def owner(cap):
    """[P] the slot of every captured point"""
    return np.repeat(np.arange(len(cap["first"]) - 1), np.diff(cap["first"]))


def kept_band(cap, c, tol=detect_law.TOL):
    """[n, M] the objects whose kept flag 3.12's band leaves out: a float64 box extreme within tol of what it is compared with"""
    n, M = cap["kept"][c].shape
    u, v, z = project64(cap, c, cap["bbox3d"].reshape(-1, 3))
    u, v, z = (a.reshape(n, M, 8) for a in (u, v, z))
    front = z > 0
    w, h = (float(x) for x in cap["cam_resolution"][c])
    ext = np.stack([np.where(front, u, np.inf).min(-1), np.where(front, v, np.inf).min(-1),
                    np.where(front, u, -np.inf).max(-1), np.where(front, v, -np.inf).max(-1)], axis=-1)
    with np.errstate(invalid="ignore"):
        return front.any(-1) & (np.abs(ext - np.array([w, h, 1.0, 1.0])) <= tol).any(-1)


def landing(cap, c, slots=None, max_depth=None, kept=None):
    """What the float64 projection says of camera c: per pose the in-image points of the kept objects (restricted to `slots`).
    Returns a list over poses of dicts: idx (point indices), x, y (integer pixels), u, v, z (float64)."""
    u, v, z = project64(cap, c)
    own = owner(cap)
    w, h = (int(x) for x in cap["cam_resolution"][c])
    kept = cap["kept"][c] if kept is None else kept
    out = []
    for i in range(u.shape[0]):
        ok = kept[i][own] & (z[i] > 0)
        if slots is not None:
            ok &= np.isin(own, slots)
        with np.errstate(invalid="ignore"):
            x, y = np.trunc(u[i]), np.trunc(v[i])
            ok &= (x >= 0) & (x < w) & (y >= 0) & (y < h)
        idx = np.nonzero(ok)[0]
        out.append(dict(idx=idx, x=x[idx].astype(int), y=y[idx].astype(int), u=u[i][idx], v=v[i][idx], z=z[i][idx]))
    return out


def fragile(cap, c, tol=TOL, tol_b=TOL_B, slots=None, max_depth=None, kept=None):
    """(hard [n, H, W], soft [n, H, W]) bool, from the float64 capture alone.  hard: an in-front point of a kept object lands in
    the pixel or beside it with its untruncated u or v within tol of an integer - or belongs to an object whose kept flag is in
    3.12's band; the pixel is not compared.  soft: the nearest point of the pixel has 255 (1 - z / max_depth) within tol_b of an
    integer; one level of difference is allowed."""
    md = float(cap["max_depth"]) if max_depth is None else float(max_depth)
    u, v, z = project64(cap, c)
    own = owner(cap)
    w, h = (int(x) for x in cap["cam_resolution"][c])
    n = u.shape[0]
    kept = cap["kept"][c] if kept is None else kept
    band = kept_band(cap, c)
    hard, soft = np.zeros((n, h, w), dtype=bool), np.zeros((n, h, w), dtype=bool)
    for i in range(n):
        sel = (kept[i] | band[i])[own] & (z[i] > 0)
        if slots is not None:
            sel &= np.isin(own, slots)
        ui, vi, zi = u[i][sel], v[i][sel], z[i][sel]
        near = (np.abs(ui - np.round(ui)) <= tol) | (np.abs(vi - np.round(vi)) <= tol) | band[i][own[sel]]
        for uu, vv in zip(ui[near], vi[near]):
            for xx in {np.trunc(uu - tol), np.trunc(uu + tol)}:
                for yy in {np.trunc(vv - tol), np.trunc(vv + tol)}:
                    if 0 <= xx < w and 0 <= yy < h:
                        hard[i, int(yy), int(xx)] = True
        x, y = np.trunc(ui), np.trunc(vi)
        inside = (x >= 0) & (x < w) & (y >= 0) & (y < h)
        zbuf = np.full((h, w), np.inf)
        np.minimum.at(zbuf, (y[inside].astype(int), x[inside].astype(int)), zi[inside])
        b = 255.0 * (1.0 - np.minimum(zbuf, md) / md)
        soft[i] = np.isfinite(zbuf) & (np.abs(b - np.round(b)) <= tol_b)
    return hard, soft


def image64(cap, c, slots=None, max_depth=None):
    """the u8 image [n, H, W] the float64 projection gives - what the reference's loop computes, vectorised; the tests hold it to the
    captured image exactly, so that the fragile pixels are marked from the right geometry"""
    md = float(cap["max_depth"]) if max_depth is None else float(max_depth)
    w, h = (int(x) for x in cap["cam_resolution"][c])
    out = []
    for L in landing(cap, c, slots):
        zbuf = np.full((h, w), np.inf)
        np.minimum.at(zbuf, (L["y"], L["x"]), L["z"])
        zz = np.where(np.isfinite(zbuf), np.clip(zbuf, 0, md), md)
        out.append((255 * (1 - zz / md)).astype(np.uint8))
    return np.array(out)


def host_points32(cap, c):
    """(u [n, P], v [n, P], z [n, P]) float32: the HOST function's own untruncated pixel coordinates and depth of every captured
    point - fpv_detect_eval in "float" mode on the degenerate box (X, X), which runs the operations of fpv_splat_point on X (the
    Targets' X = vertex + offset is formed in float32 first, like the kernel does)"""
    from fpyv_amd.camera import Camera
    from fpyv_amd.detect import BoxDetector
    cl = cloud(cap)
    X = np.vstack([cl.world_points(k) for k in range(cl.count)]).astype(np.float32)
    cam = Camera(float(cap["cam_angle"][c]), cap["cam_rel"][c], [int(x) for x in cap["cam_resolution"][c]], fov=float(cap["cam_fov"][c]))
    det = BoxDetector(camera=cam, pixels="float")
    n = cap["p"].shape[0]
    u, v, z = (np.zeros((n, X.shape[0]), dtype=np.float32) for _ in range(3))
    for a in range(0, X.shape[0], 72):
        b = min(a + 72, X.shape[0])
        got = det.evaluate(cap["p"], cap["q"], boxes=np.hstack([X[a:b], X[a:b]]))
        u[:, a:b], v[:, a:b], z[:, a:b] = got["boxes"][:, 0, :].T, got["boxes"][:, 1, :].T, got["depth"].T
    return u, v, z


def measure(cap):
    """the guard bands of a capture against this build's fp32 host function, and what they leave out"""
    rep, err, err_b = {}, 0.0, 0.0
    md = np.float32(cap["max_depth"])
    for c in range(cap["proj"].shape[0]):
        u32, v32, z32 = host_points32(cap, c)
        u, v, z = project64(cap, c)
        w, h = (int(x) for x in cap["cam_resolution"][c])
        with np.errstate(invalid="ignore"):
            inside = (z > 0) & (np.trunc(u) >= 0) & (np.trunc(u) < w) & (np.trunc(v) >= 0) & (np.trunc(v) < h)
        err = max(err, float(np.abs(u32.astype(np.float64) - u)[inside].max()), float(np.abs(v32.astype(np.float64) - v)[inside].max()))
        near = inside & (z < float(md))
        b32 = np.float32(255.0) * (np.float32(1.0) - z32 / md)                 # fpv_depth_u8's two operations, in float32
        err_b = max(err_b, float(np.abs(b32.astype(np.float64) - 255.0 * (1.0 - z / float(md)))[near].max()))
        rep[f"camera {c}: in-image points"] = int(inside.sum())
    tol, tol_b = 4.0 * err, 4.0 * err_b
    rep["tol (pixels)"], rep["tol_b (levels)"] = f"{tol:.4e}", f"{tol_b:.4e}"
    for c in range(cap["proj"].shape[0]):
        hard, soft = fragile(cap, c, tol, tol_b)
        rep[f"camera {c}: fragile share"] = f"{float((hard | soft).mean()):.5f} (hard {int(hard.sum())}, soft {int(soft.sum())} of {hard.size})"
        rep[f"camera {c}: lit share"] = f"{float((cap[f'image{c}'] > 0).mean()):.4f}"
        rep[f"camera {c}: kept flags in 3.12's band"] = int(kept_band(cap, c).sum())
    return rep


def compare(cap, c, got, want, hard, soft):
    """holds a u8 image [n, H, W] to the captured one: exact outside the fragile pixels, one level on the soft ones.  Returns the
    number of pixels compared exactly."""
    got, want = np.asarray(got).astype(np.int64), np.asarray(want).astype(np.int64)
    exact = ~hard & ~soft
    bad = exact & (got != want)
    assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[:5].tolist())
    one = soft & ~hard
    assert np.all(np.abs(got[one] - want[one]) <= 1)
    return int(exact.sum())
