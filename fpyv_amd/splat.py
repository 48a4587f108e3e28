"""Point-cloud camera: the reference's splatted depth image - `Camera.render_depth_image`, `render_image` and the lit-pixel centroid
its tracker steers by (src/utils/components.py:602-629, src/core/simulator.py:102-107) - for N drones, and the kernel's
own point and pixel functions on the host.

`PointCloudCamera` holds the camera (the reference's `Camera` arguments under the depth camera's limits: W, H in 4..128, W a multiple
of 4), `max_depth`, the encoding - "u8" the reference's image byte, "metres" the float32 depth, "mask" `render_image`'s 0 / 1 - and
whether the centroid is wanted.  `DroneBatch(cloud_camera=cam)` renders in one kernel: `batch.render_points(object_list)` fills
`batch.points_image` [num_envs, H, W] and, with `centroid=True`, `batch.points_centroid` [num_envs, 2] (x, y; NaN where nothing is
lit - the value `calculate_needed_force_orientation(pixel=)` takes as "not guided") and `batch.points_lit` [num_envs]
(include/fpv_abi.h "Point-cloud camera").
"""
from __future__ import annotations

import ctypes as C
from typing import Any, Optional, Sequence

import numpy as np

from . import _lib
from .clouds import PointCloud
from .rays import poses


class PointCloudCamera:
    def __init__(self, resolution: Sequence[int] = (64, 48), fov: float = 120.0, camera_angle: float = 35.0,
                 position_relative_to_frame: Sequence[float] = (0.1, 0.0, 0.0), max_depth: float = 25.0, encoding: str = "u8",
                 centroid: bool = False):
        if encoding not in _lib.SPLAT_ENCODINGS:
            raise ValueError(f'encoding must be "u8", "metres" or "mask", got {encoding!r}')
        self.resolution = (int(resolution[0]), int(resolution[1]))
        self.fov, self.camera_angle = float(fov), float(camera_angle)
        self.relative_position = np.asarray(position_relative_to_frame, dtype=np.float64).reshape(3)
        self.max_depth, self.encoding, self.centroid = float(max_depth), encoding, bool(centroid)

    @property
    def dtype(self) -> Any:
        return np.float32 if self.encoding == "metres" else np.uint8

    def derive(self) -> "_lib.FpvSplat":
        """fpv_splat_derive: a fresh fpv_splat_t holding the camera numbers, max_depth and the encoding; the cloud and the pointers
        are the caller's to fill - host arithmetic, no device.  Raises FpvError naming what it refuses."""
        cam = _lib.FpvCamera()
        cam.pitch_deg, cam.fov_deg = self.camera_angle, self.fov
        cam.width, cam.height = self.resolution
        cam.relative_position[:] = [float(x) for x in self.relative_position]
        s = _lib.FpvSplat()
        _lib.check(_lib.lib().fpv_splat_derive(C.byref(cam), C.byref(s)))
        s.struct_size = C.sizeof(_lib.FpvSplat)
        s.max_depth, s.encoding = self.max_depth, _lib.SPLAT_ENCODINGS[self.encoding]
        return s

    def evaluate(self, p: Any, q: Any, cloud: Any, image_ld: Optional[int] = None) -> dict:
        """fpv_splat_eval: the kernel's own functions on the host, for n drones at once.  p [n, 3], q [n, 4] (wxyz), `cloud` a
        PointCloud or an object list (`PointCloud.from_world`).  `image_ld` (>= W * H, a multiple of 4; default W * H) is the stride
        between drones evaluated into.  Returns a dict: image [n, H, W] (uint8, or float32 for "metres"), and - `centroid=True` -
        centroid [n, 2] float32 (x, y) and lit [n] int32, else None."""
        pp, qq = poses(p, q)
        n = pp.shape[0]
        if not isinstance(cloud, PointCloud):
            cloud = PointCloud.from_world(cloud)
        s = self.derive()
        cloud.fill(s)
        s.points = cloud.points.ctypes.data
        w, h = self.resolution
        ld = w * h if image_ld is None else int(image_ld)
        out = np.zeros((max(n, 1), max(ld, 1)), dtype=self.dtype)
        s.image, s.image_ld = out.ctypes.data, ld
        cen = lit = None
        if self.centroid:
            cen, lit = np.zeros((max(n, 1), 2), dtype=np.float32), np.zeros(max(n, 1), dtype=np.int32)
            s.centroid, s.lit = cen.ctypes.data, lit.ctypes.data
        _lib.check(_lib.lib().fpv_splat_eval(C.byref(s), n, pp.ctypes.data, qq.ctypes.data))
        return dict(image=out[:n, :w * h].reshape(n, h, w), centroid=None if cen is None else cen[:n], lit=None if lit is None else lit[:n])
