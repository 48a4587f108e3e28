"""Depth camera: the reference's FPV camera as a batched sensor, and the render kernel's own pixel function on the host.

`DepthCamera` holds what the reference's `Camera(camera_pitch_angle, position_relative_to_frame, resolution, fov)` holds, plus
the reach and the encoding of a depth image.  `DroneBatch(depth_camera=cam)` renders one image per drone of the collision world
and the gates: `batch.render_depth(object_list)` fills `batch.depth` [num_envs, H, W] (include/fpv_abi.h "Depth camera").
"""
from __future__ import annotations

import ctypes as C
from typing import Any, Sequence

import numpy as np

from . import _lib
from .objects import to_rows
from .rays import poses


class DepthCamera:
    """A pinhole camera fixed to the drone's frame: `camera_angle` degrees of pitch, `fov` degrees across the image width,
    `resolution` (W, H) with 4 <= W, H <= 128 and W a multiple of 4.  A pixel reports the z-depth (the reference's
    `projection_matrix @ point` third row) of the nearest Ground / Cylinder / Target / gate frame, at most `max_depth`; `encoding`
    "metres" gives float32, "u8" the reference's image byte `uint8(255 (1 - depth / max_depth))`.  `gate_frame` is the width of
    the frame a gate is drawn with around its aperture."""

    def __init__(self, resolution: Sequence[int] = (64, 48), fov: float = 120.0, camera_angle: float = 35.0,
                 position_relative_to_frame: Sequence[float] = (0.1, 0.0, 0.0), max_depth: float = 25.0, encoding: str = "metres",
                 gate_frame: float = 0.15):
        if encoding not in _lib.DEPTH_ENCODINGS:
            raise ValueError(f'encoding must be "metres" or "u8", got {encoding!r}')
        self.resolution = (int(resolution[0]), int(resolution[1]))
        self.fov, self.camera_angle = float(fov), float(camera_angle)
        self.relative_position = np.asarray(position_relative_to_frame, dtype=np.float64).reshape(3)
        self.max_depth, self.encoding, self.gate_frame = float(max_depth), encoding, float(gate_frame)
        self._derived = None

    @classmethod
    def from_params(cls, params: Any, resolution: Any = None, **kw: Any) -> "DepthCamera":
        """From the reference's params (a yaml path or the loaded dict): its `camera:` section gives camera_angle,
        position_relative_to_frame and fov; `resolution` replaces the section's (the reference's 640 x 480 is beyond an image here)."""
        if not isinstance(params, dict):
            import yaml
            with open(params, encoding="utf-8") as f:
                params = yaml.safe_load(f)
        c = params["camera"]
        return cls(resolution=resolution if resolution is not None else c["resolution"], fov=c["fov"], camera_angle=c["camera_angle"],
                   position_relative_to_frame=c["position_relative_to_frame"], **kw)

    def derive(self) -> "_lib.FpvDepthRender":
        """fpv_camera_derive: a fresh fpv_depth_render_t holding the direction vectors, the offset, dir_len_max, the focal length
        and the relative rotation of this camera, max_depth, the encoding and the frame width (`image`, `objects` and the gates
        are the caller's to fill) - host arithmetic, no device.  Raises FpvError (FPV_EPARAM) naming what it refuses."""
        cam = _lib.FpvCamera()
        cam.pitch_deg, cam.fov_deg, cam.width, cam.height = self.camera_angle, self.fov, self.resolution[0], self.resolution[1]
        cam.relative_position[:] = [float(x) for x in self.relative_position]
        s = _lib.FpvDepthRender()
        _lib.check(_lib.lib().fpv_camera_derive(C.byref(cam), C.byref(s)))
        s.struct_size, s.max_depth, s.encoding = C.sizeof(_lib.FpvDepthRender), self.max_depth, _lib.DEPTH_ENCODINGS[self.encoding]
        s.gate_frame_width = self.gate_frame
        self._derived = s
        return _lib.FpvDepthRender.from_buffer_copy(s)

    def _d(self) -> "_lib.FpvDepthRender":
        if self._derived is None:
            self.derive()
        return self._derived

    @property
    def focal_length(self) -> float:
        return float(self._d().focal_length)

    @property
    def relative_rotation_matrix(self) -> np.ndarray:
        return np.array(self._d().relative_rotation[:], dtype=np.float64).reshape(3, 3)

    @property
    def intrinsic_matrix(self) -> np.ndarray:
        f, (w, h) = self.focal_length, self.resolution
        return np.array([[f, 0.0, w / 2], [0.0, f, h / 2], [0.0, 0.0, 1.0]])

    @property
    def dtype(self) -> Any:
        return np.uint8 if self.encoding == "u8" else np.float32

    def evaluate(self, p: Any, q: Any, object_list: Sequence[Any] = (), gates: Any = ()) -> np.ndarray:
        """fpv_depth_eval: the render kernel's own pixel function on the host, for n drones at once.  p [n, 3], q [n, 4] (wxyz),
        `object_list` what `step` takes (or raw rows), `gates` a list of gates or their [count, 16] descriptor rows
        (`fpyv_amd.gates.derive`).  Returns the images [n, H, W], float32 or uint8."""
        pp, qq = poses(p, q)
        n = pp.shape[0]
        s = self.derive()
        objs = _lib.pack_objects(to_rows(object_list or ()))
        s.objects = C.addressof(objs)
        rows = gate_rows(gates)
        if rows is not None:
            s.gate_descriptors, s.gate_count = rows.ctypes.data, rows.shape[0]
        w, h = self.resolution
        out = np.zeros((n, h, w), dtype=self.dtype)
        s.image, s.image_stride = out.ctypes.data, w * h
        _lib.check(_lib.lib().fpv_depth_eval(C.byref(s), n, pp.ctypes.data, qq.ctypes.data))
        return out


def gate_rows(gates: Any):
    """[count, 16] float32 descriptor rows, 16-byte aligned, of a list of gates or of rows already derived; None for no gates"""
    if gates is None:
        return None
    if isinstance(gates, np.ndarray) and gates.dtype == np.float32 and gates.ndim == 2:
        rows = gates
    else:
        gates = list(gates)
        if not gates:
            return None
        from .gates import derive
        rows = derive(gates)
    if rows.shape[0] == 0:
        return None
    buf = np.zeros(rows.size + 4, dtype=np.float32)
    off = (-buf.ctypes.data % 16) // 4
    al = buf[off:off + rows.size].reshape(rows.shape)
    al[...] = rows
    return al


class Camera(DepthCamera):
    """The reference's constructor signature (components.py:450): Camera(camera_pitch_angle, position_relative_to_frame,
    resolution, fov=None, focal_length=None); one of fov and focal_length is given."""

    def __init__(self, camera_pitch_angle: float, position_relative_to_frame: Sequence[float], resolution: Sequence[int],
                 fov: Any = None, focal_length: Any = None, **kw: Any):
        if fov is None:
            if focal_length is None:
                raise ValueError("a camera needs fov= or focal_length=")
            fov = float(np.rad2deg(2 * np.arctan(resolution[0] / (2 * focal_length))))
        super().__init__(resolution=resolution, fov=fov, camera_angle=camera_pitch_angle,
                         position_relative_to_frame=position_relative_to_frame, **kw)
