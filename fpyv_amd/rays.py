"""Range sensor: ray sets in the body frame and the scan kernel's own lane function on the host.

A ray set is 1..32 unit directions in the drone's body frame (x forward, y left, z up).  `DroneBatch(range_rays=rays,
range_max=20.0)` scans them against the collision world: `batch.range_scan(object_list)` gives, per ray and drone, the distance
to the nearest Ground / Cylinder / Target along `R(q) d_b`, at most `range_max` (include/fpv_abi.h "Range scan").
"""
from __future__ import annotations

import ctypes as C
from typing import Any, Sequence

import numpy as np

from . import _lib
from .objects import to_rows


def derive(dirs: Any) -> np.ndarray:
    """[R, 3] float32 unit directions by fpv_rays_derive (normalised in double, narrowed once) - host arithmetic, no device.
    Raises FpvError (FPV_EPARAM) naming the ray for a zero or non-finite direction or a count outside 1..32."""
    d = np.ascontiguousarray(np.asarray(dirs, dtype=np.float64).reshape(-1, 3))
    out = np.zeros((max(1, d.shape[0]), 3), dtype=np.float32)
    _lib.check(_lib.lib().fpv_rays_derive(d.shape[0], d.ctypes.data, out.ctypes.data))
    return out


def fan(count: int, fov_deg: float, pitch_deg: float = 0.0) -> np.ndarray:
    """`count` rays spread evenly over `fov_deg` in the body's horizontal plane, centred on body +x (the first ray looks left,
    + fov / 2 of yaw about +z), all tilted up by `pitch_deg`.  One ray looks straight ahead."""
    if not 1 <= int(count) <= _lib.FPV_MAX_RAYS:
        raise ValueError(f"a ray set has 1..{_lib.FPV_MAX_RAYS} rays")
    yaw = np.deg2rad(np.linspace(0.5 * fov_deg, -0.5 * fov_deg, int(count)) if count > 1 else np.zeros(1))
    pitch = np.deg2rad(float(pitch_deg))
    return derive(np.stack([np.cos(pitch) * np.cos(yaw), np.cos(pitch) * np.sin(yaw), np.full_like(yaw, np.sin(pitch))], axis=1))


def grid(cols: int, rows: int, hfov_deg: float, vfov_deg: float) -> np.ndarray:
    """A depth-image-like grid, row-major from the top-left pixel: pinhole rays through the pixel centres of a `cols` x `rows`
    image plane at distance 1 along body +x that spans `hfov_deg` x `vfov_deg`; cols * rows <= 32."""
    if cols < 1 or rows < 1 or cols * rows > _lib.FPV_MAX_RAYS:
        raise ValueError(f"a grid has 1..{_lib.FPV_MAX_RAYS} rays (cols * rows)")
    if not (0.0 < hfov_deg < 180.0 and 0.0 < vfov_deg < 180.0):
        raise ValueError("a pinhole grid needs fields of view in (0, 180) degrees")
    w, h = np.tan(np.deg2rad(0.5 * hfov_deg)), np.tan(np.deg2rad(0.5 * vfov_deg))
    y = w * (1.0 - (2.0 * np.arange(cols) + 1.0) / cols)         # left (+y) to right
    z = h * (1.0 - (2.0 * np.arange(rows) + 1.0) / rows)         # top (+z) to bottom
    zz, yy = np.meshgrid(z, y, indexing="ij")
    return derive(np.stack([np.ones(cols * rows), yy.reshape(-1), zz.reshape(-1)], axis=1))


def poses(p: Any, q: Any):
    """The drones a host evaluation (`evaluate`, `DepthCamera.evaluate`) is given, as contiguous float32 p [n, 3] and q [n, 4]"""
    pp, qq = (np.ascontiguousarray(np.asarray(a, dtype=np.float32).reshape(-1, w)) for a, w in ((p, 3), (q, 4)))
    if qq.shape[0] != pp.shape[0]:
        raise ValueError("p and q must describe the same n drones")
    return pp, qq


def evaluate(rays: Any, max_range: float, p: Any, q: Any, object_list: Sequence[Any] = ()) -> np.ndarray:
    """fpv_range_eval: the scan kernel's own lane function on the host, for n drones at once.  `rays` [R, 3] (`derive`), p [n, 3],
    q [n, 4] (wxyz), `object_list` what `step` takes (or raw rows).  Returns the ranges [R, n] float32."""
    pp, qq = poses(p, q)
    n = pp.shape[0]
    s = _lib.pack_range_scan(np.asarray(rays, dtype=np.float32).reshape(-1, 3), max_range)
    objs = _lib.pack_objects(to_rows(object_list or ()))
    s.objects = C.addressof(objs)
    ld = (n + 3) // 4 * 4
    out = np.zeros((s.ray_count, ld), dtype=np.float32)
    s.ranges, s.ranges_ld = out.ctypes.data, ld
    _lib.check(_lib.lib().fpv_range_eval(C.byref(s), n, pp.ctypes.data, qq.ctypes.data))
    return np.ascontiguousarray(out[:, :n])
