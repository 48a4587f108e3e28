"""What the detection tests share: the g22 capture of the reference's bounding boxes (tools/gen_detect_golden.py), the scene and the
cameras it describes as this package's objects, the float64 boxes the capture implies, and the guard-band comparison of an fp32
result with them (tests/test_detect_host.py on the host function, tests/test_gpu_detect.py on the kernel).  Nothing here is used
by the product."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g22_bbox.npz")
# 4 x the largest |fp32 "float"-mode box extreme - float64 extreme| over the g22 capture (measure() below), pixels
TOL = 6.61e-3         # measured 6.607e-3 (largest error 1.652e-3 pixels, on the 640 x 480 camera)
SHAPES = ("rectangle", "circle", "half_circle")
_cache = {}


def load():
    if "cap" not in _cache:
        with np.load(GOLDEN) as z:
            _cache["cap"] = {k: z[k] for k in z.files}
    return _cache["cap"]


def scene(cap):
    """(object_list, gates) of the capture; slot order ground, cylinders, spheres, then the gates"""
    from fpyv_amd.objects import Cylinder, Gate, Ground, Target
    objs = [Ground(float(cap["ground_size"]), 4)]
    objs += [Cylinder(p, float(r), float(h), 17, 5) for p, r, h in zip(cap["cyl_position"], cap["cyl_radius"], cap["cyl_height"])]
    objs += [Target(p, float(r)) for p, r in zip(cap["sph_position"], cap["sph_radius"])]
    gates = [Gate(p, R, float(s), shape=SHAPES[int(k)], resolution=17)
             for p, R, s, k in zip(cap["gate_position"], cap["gate_rotation"], cap["gate_size"], cap["gate_shape"])]
    return objs, gates


def detector(cap, c, pixels="int", **kw):
    from fpyv_amd.camera import Camera
    from fpyv_amd.detect import BoxDetector
    cam = Camera(float(cap["cam_angle"][c]), cap["cam_rel"][c], [int(x) for x in cap["cam_resolution"][c]], fov=float(cap["cam_fov"][c]))
    return BoxDetector(camera=cam, pixels=pixels, **kw)


def extremes64(cap, c):
    """the float64 untruncated box [n, M, 4] (x_min, y_min, x_max, y_max) over the in-front corners of camera c (NaN with none in
    front), the smallest in-front depth [n, M] and the in-front count [n, M]"""
    uv, d = cap["uv"][c], cap["depth"][c]
    front = d > 0
    lo = np.where(front[..., None], uv, np.inf).min(axis=-2)
    hi = np.where(front[..., None], uv, -np.inf).max(axis=-2)
    ext = np.concatenate([lo, hi], axis=-1)
    none = ~front.any(axis=-1)
    ext[none] = np.nan
    dmin = np.where(front, d, np.inf).min(axis=-1)
    dmin[none] = np.nan
    return ext, dmin, front.sum(axis=-1)


def thresholds(cap, c, pixels):
    """what each extreme is compared with for `visible`: x_min < W, y_min < H, x_max > 0, y_max > 0 - on truncated integers the
    last two read `>= 1`"""
    w, h = (float(x) for x in cap["cam_resolution"][c])
    one = 1.0 if pixels == "int" else 0.0
    return np.array([w, h, one, one])


def visible64(cap, c, pixels):
    ext, _, cnt = extremes64(cap, c)
    w, h = (float(x) for x in cap["cam_resolution"][c])
    e = np.trunc(ext) if pixels == "int" else ext
    with np.errstate(invalid="ignore"):
        return (cnt > 0) & (e[..., 2] > 0) & (e[..., 3] > 0) & (e[..., 0] < w) & (e[..., 1] < h)


def near_threshold(cap, c, pixels, tol):
    ext, _, cnt = extremes64(cap, c)
    with np.errstate(invalid="ignore"):
        return (cnt > 0) & (np.abs(ext - thresholds(cap, c, pixels)) <= tol).any(axis=-1)


def near_integer(cap, c, tol):
    ext, _, cnt = extremes64(cap, c)
    with np.errstate(invalid="ignore"):
        return (cnt > 0)[..., None] & (np.abs(ext - np.round(ext)) <= tol)


def measure(cap):
    """(4 x the largest |fp32 float-mode extreme - float64 extreme|, the share of the coordinates the band of that width leaves out
    of the exact comparison, the share of the visible flags it leaves out), over both cameras"""
    objs, gates = scene(cap)
    err = 0.0
    for c in range(cap["uv"].shape[0]):
        got = detector(cap, c, "float").evaluate(cap["p"], cap["q"], objs, gates)
        ext, _, cnt = extremes64(cap, c)
        b = np.transpose(got["boxes"], (2, 0, 1)).astype(np.float64)
        err = max(err, float(np.abs(b - ext)[cnt > 0].max()))
    tol = 4.0 * err
    coords = np.concatenate([near_integer(cap, c, tol).ravel() for c in range(cap["uv"].shape[0])])
    flags = np.concatenate([(near_threshold(cap, c, "int", tol) | near_threshold(cap, c, "float", tol)).ravel() for c in range(cap["uv"].shape[0])])
    return tol, float(coords.mean()), float(flags.mean())


def check_against_capture(cap, c, pixels, got, tol=TOL):
    """The guard-band comparison of a result of camera c - boxes [M, 4, n], depth [M, n], visible [M, n] - with the capture.
    Returns (coordinates compared, coordinates left out, flags compared, flags left out)."""
    ext, dmin, cnt = extremes64(cap, c)
    b = np.transpose(np.asarray(got["boxes"]), (2, 0, 1)).astype(np.float64)
    d = np.asarray(got["depth"]).T.astype(np.float64)
    v = np.asarray(got["visible"]).T.astype(bool)
    some = cnt > 0
    # the zero rule: nothing in front
    assert np.all(b[~some] == 0.0) and np.all(d[~some] == 0.0) and not v[~some].any()
    assert np.all(d[some] > 0.0)
    # depth = a column of Rcam . (X - pcam) in fp32: differences of coordinates up to 90 m (half an ulp each, 3.8e-6), three products
    # summed, Rcam's entries good to 2 ulps of 1 (2.4e-7 x 90 m): 5e-5 m bounds the sum of those
    np.testing.assert_allclose(d[some], dmin[some], rtol=0, atol=5e-5)
    if pixels == "float":
        assert np.abs(b - ext)[some].max() <= tol
        band_c = np.zeros_like(ext, dtype=bool)
    else:
        want = np.trunc(ext)
        has = cap["has_bbox2d"][c]
        assert np.array_equal(has, some)
        assert np.array_equal(want[has], cap["bbox2d"][c][has].astype(np.float64))          # the reference's own integers
        band_c = near_integer(cap, c, tol)
        exact = some[..., None] & ~band_c
        assert np.array_equal(b[exact], want[exact])
        assert np.all(np.abs(b[band_c] - want[band_c]) <= 1.0)
    want_v = visible64(cap, c, pixels)
    if pixels == "int":
        assert np.array_equal(want_v, cap["kept"][c])                                       # the reference's own pruning
    band_v = near_threshold(cap, c, pixels, tol)
    assert np.array_equal(v[~band_v], want_v[~band_v])
    return int(some.sum()) * 4, int(band_c.sum()), int(v.size), int(band_v.sum())
