"""Object detections: the 2-D bounding box of every object and gate in every drone's camera - the reference's
`Camera.project(attr='bbox3d')`, `bbox3d_to_bbox2d`, `bbox2d` and `pruned_objects_list` (/root/reference/src/utils/components.py:558-600)
over the boxes of `helper_functions.bbox3d` (helper_functions.py:120-136) - for N drones, and the kernel's own lane function on the host.

`BoxDetector` holds the camera (the reference's `Camera` arguments - no image is written, so its 640 x 480 is fine), the pixel mode,
the clip flag and the resolution the gates' corner points are taken at.  `DroneBatch(detector=det)` detects in one kernel:
`batch.detect(object_list)` fills `batch.boxes` [M, 4, num_envs], `batch.box_depth` [M, num_envs] and `batch.box_visible`
[M, num_envs]; slot order is the collidable entries of the object list, then the gates of the course, then - with `own_target=True`
and a pursuit task - the drone's own target (include/fpv_abi.h "Object detections").
"""
from __future__ import annotations

import ctypes as C
from typing import Any, Optional, Sequence

import numpy as np

from . import _lib
from .camera import DepthCamera
from .gates import _rows_of
from .objects import to_rows
from .rays import poses


class BoxDetector:
    """`camera`: a DepthCamera / Camera, None = the `camera` section of the packaged parameters.  `pixels` "int" truncates every
    pixel coordinate toward zero like the reference's astype(int) (the values stay float32), "float" keeps the sub-pixel value.
    `clip=True` clamps a visible box to the image (the reference does not).  `gate_resolution` is the number of points of a round
    gate's outline (the reference's Gate(resolution=17)).  `own_target=True` adds the drone's own pursuit target as the last slot."""

    def __init__(self, camera: Optional[DepthCamera] = None, pixels: str = "int", clip: bool = False, gate_resolution: int = 17,
                 own_target: bool = False):
        if pixels not in _lib.DETECT_PIXELS:
            raise ValueError(f'pixels must be "int" or "float", got {pixels!r}')
        if int(gate_resolution) < 1:
            raise ValueError("gate_resolution must be >= 1")
        if camera is None:
            from .params import load_params
            c = load_params().camera
            camera = DepthCamera(resolution=c["resolution"], fov=c["fov"], camera_angle=c["camera_angle"],
                                 position_relative_to_frame=c["position_relative_to_frame"])
        self.camera, self.pixels, self.clip = camera, pixels, bool(clip)
        self.gate_resolution, self.own_target = int(gate_resolution), bool(own_target)

    def derive(self) -> "_lib.FpvDetect":
        """fpv_detect_derive: a fresh fpv_detect_t holding the camera numbers, the pixel mode and the clip flag; the table and the
        pointers are the caller's to fill - host arithmetic, no device.  Raises FpvError naming what it refuses."""
        cam = _lib.FpvCamera()
        cam.pitch_deg, cam.fov_deg = self.camera.camera_angle, self.camera.fov
        cam.width, cam.height = self.camera.resolution
        cam.relative_position[:] = [float(x) for x in self.camera.relative_position]
        s = _lib.FpvDetect()
        _lib.check(_lib.lib().fpv_detect_derive(C.byref(cam), C.byref(s)))
        s.struct_size = C.sizeof(_lib.FpvDetect)
        s.pixel_mode, s.clip = _lib.DETECT_PIXELS[self.pixels], int(self.clip)
        return s

    def table(self, object_list: Sequence[Any] = (), gates: Sequence[Any] = ()) -> "_lib.FpvBoxes":
        """fpv_boxes_derive: the fpv_boxes_t of the collidable entries of `object_list` (objects.to_rows order) followed by `gates`
        in order.  A Ground must carry its `size`: a raw row, or `Ground()` with its default 0, is refused by name."""
        objs = [o for o in (object_list or ()) if not (getattr(o, "collides", True) is False or type(o).__name__ in ("Gate", "Trail"))]
        rows = to_rows(objs)
        packed = _lib.pack_objects(rows)
        sizes = (C.c_double * max(1, len(rows)))()
        for k, (o, r) in enumerate(zip(objs, rows)):
            sizes[k] = float(getattr(o, "size", 0.0) or 0.0) if int(r[0]) == _lib.OBJ_GROUND else 0.0
        gates = list(gates or ())
        if len(gates) > _lib.FPV_MAX_GATES:
            raise ValueError(f"at most {_lib.FPV_MAX_GATES} gates")
        arr = _rows_of(gates)
        out = _lib.FpvBoxes()
        _lib.check(_lib.lib().fpv_boxes_derive(C.addressof(packed), C.addressof(sizes), C.addressof(arr) if gates else None, len(gates),
                                               self.gate_resolution, C.byref(out)))
        return out

    def boxes(self, object_list: Sequence[Any] = (), gates: Sequence[Any] = ()) -> np.ndarray:
        """[M, 6] float32 (min x, y, z, max x, y, z): the box table of `object_list` and `gates` in slot order"""
        t = self.table(object_list, gates)
        return np.array([list(t.box[m]) for m in range(t.count)], dtype=np.float32).reshape(t.count, 6)

    def evaluate(self, p: Any, q: Any, object_list: Sequence[Any] = (), gates: Sequence[Any] = (), target_rows: Any = None,
                 target_radius: Any = 0.0, boxes: Any = None, ld: Optional[int] = None) -> dict:
        """fpv_detect_eval: the kernel's own lane function on the host, for n drones at once.  p [n, 3], q [n, 4] (wxyz); the slots
        are `boxes` [M, 6] when given (raw rows: anything finite with min <= max), else the table of `object_list` and `gates`;
        `target_rows` [3, n] adds every drone's own box, centre +- `target_radius` (a number, or [n]) as the last slot.  `ld`
        (>= n, a multiple of 4; default n rounded up) is the row stride evaluated into.  Returns a dict: boxes [M, 4, n] float32
        (x_min, y_min, x_max, y_max), depth [M, n] float32, visible [M, n] bool."""
        pp, qq = poses(p, q)
        n = pp.shape[0]
        s = self.derive()
        if boxes is not None:
            b = np.asarray(boxes, dtype=np.float32).reshape(-1, 6)
            t = _lib.FpvBoxes()
            t.count = b.shape[0]                                # (too many: the library refuses the count before it reads a box)
            for m in range(min(b.shape[0], _lib.FPV_MAX_BOXES)):
                t.box[m][:] = [float(x) for x in b[m]]
        else:
            t = self.table(object_list, gates)
        s.table = C.addressof(t)
        keep = [t]
        m = t.count
        if target_rows is not None:
            tr = np.ascontiguousarray(np.asarray(target_rows, dtype=np.float32).reshape(3, n))
            s.target_rows, s.target_ld = tr.ctypes.data, n
            keep.append(tr)
            if np.ndim(target_radius) == 0:
                s.target_radius_all = float(target_radius)
            else:
                rad = np.ascontiguousarray(np.asarray(target_radius, dtype=np.float32).reshape(n))
                s.target_radius = rad.ctypes.data
                keep.append(rad)
            m += 1
        ld = (n + 3) // 4 * 4 if ld is None else int(ld)
        rows = max(m, 1)
        out = np.zeros((rows, 4, max(ld, 1)), dtype=np.float32)
        depth = np.zeros((rows, max(ld, 1)), dtype=np.float32)
        vis = np.zeros((rows, max(ld, 1)), dtype=np.uint8)
        s.boxes, s.box_depth, s.box_visible, s.ld = out.ctypes.data, depth.ctypes.data, vis.ctypes.data, ld
        _lib.check(_lib.lib().fpv_detect_eval(C.byref(s), n, pp.ctypes.data, qq.ctypes.data))
        return dict(boxes=out[:m, :, :n], depth=depth[:m, :n], visible=vis[:m, :n].astype(bool))
