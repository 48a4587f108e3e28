"""Target chase: the reference's vision guidance law `Drone.calculate_needed_force_orientation(pixel, target, ref_frame, mode)`
(/root/reference/src/utils/components.py:258-304) for N drones, and the kernel's own lane function on the host.

`ChaseGuidance` holds what the law reads besides the drones: the camera (the reference's `Camera` arguments - no image is written,
so its 640 x 480 is fine), the five constants of params.yaml (`point_and_shoot.*`, `drone.keep_distance`,
`drone.UWB_sensor_max_range`), the mass, the guidance PID's constants, the frame and the mode.  `DroneBatch` builds one on first
use: `batch.calculate_needed_force_orientation(pixel, target)` runs the law in one kernel and returns tensors that go straight back
into `batch.step(..., rotation_matrix=, thrust_force=)` (include/fpv_abi.h "Target chase").
"""
from __future__ import annotations

import ctypes as C
from typing import Any, Optional, Tuple

import numpy as np

from . import _lib
from .camera import DepthCamera
from .rays import poses


def target_row(target: Any) -> Tuple[np.ndarray, float]:
    """(centre [3] float32, radius) of a Target (anything with `.position` and `.radius`) or of a (centre, radius) pair"""
    if hasattr(target, "position"):
        c, r = target.position, getattr(target, "radius", 0.0)
    else:
        c, r = target
    return np.asarray(c, dtype=np.float32).reshape(3), float(np.float32(r))


class ChaseGuidance:
    """The law's uniform inputs.  `params` is a DroneParams (mass, dt, keep_distance, UWB_sensor_max_range, point_and_shoot,
    force_multiplier_pid with the 5 % / full throttle forces as its output limits, camera); `camera` a DepthCamera / Camera
    replacing the params' own; `ref_frame` "world" | "drone", `mode` "level" | "frontarget"; `max_depth` the reach of the
    reference's target-only image (simulator.py:102)."""

    def __init__(self, params: Any, camera: Optional[DepthCamera] = None, ref_frame: str = "world", mode: str = "level",
                 max_depth: float = 15.0):
        if ref_frame not in _lib.CHASE_FRAMES:
            raise ValueError("Unknown reference frame")                          # components.py:278
        if mode not in _lib.CHASE_MODES:
            raise ValueError("Unknown mode")                                     # components.py:301
        self.params, self.ref_frame, self.mode, self.max_depth = params, ref_frame, mode, float(max_depth)
        if camera is None:
            c = params.camera
            camera = DepthCamera(resolution=c["resolution"], fov=c["fov"], camera_angle=c["camera_angle"],
                                 position_relative_to_frame=c["position_relative_to_frame"])
        self.camera = camera

    def pid_params(self) -> "_lib.FpvPidParams":
        """Drone.force_multiplier_pid's constants (components.py:143-145): min / max output are the 5 % and full throttle forces"""
        p = _lib.FpvPidParams()
        p.struct_size = C.sizeof(_lib.FpvPidParams)
        kw = dict(self.params.force_multiplier_pid)
        p.kP, p.kI, p.kD, p.dt = float(kw["kP"]), float(kw["kI"]), float(kw["kD"]), float(self.params.dt)
        p.integral_clip = float(kw.get("integral_clip", 1.0))
        p.min_output, p.max_output = float(self.params.min_throttle_in_force), float(self.params.max_throttle_in_force)
        p.derivative_transition_rate = float(kw.get("derivative_transition_rate", 0.5))
        return p

    def derive(self, target: Any = None) -> "_lib.FpvChase":
        """fpv_chase_derive: a fresh fpv_chase_t holding the camera numbers, the constants, the frame, the mode and - when given -
        the target (the pointers are the caller's to fill) - host arithmetic, no device.  Raises FpvError naming what it refuses."""
        cam = _lib.FpvCamera()
        cam.pitch_deg, cam.fov_deg = self.camera.camera_angle, self.camera.fov
        cam.width, cam.height = self.camera.resolution
        cam.relative_position[:] = [float(x) for x in self.camera.relative_position]
        s = _lib.FpvChase()
        _lib.check(_lib.lib().fpv_chase_derive(C.byref(cam), C.byref(s)))
        s.struct_size = C.sizeof(_lib.FpvChase)
        s.ref_frame, s.mode, s.max_depth = _lib.CHASE_FRAMES[self.ref_frame], _lib.CHASE_MODES[self.mode], self.max_depth
        p, law = self.params, self.params.point_and_shoot
        s.mass = float(p.mass)
        s.virtual_drag_coefficient, s.virtual_lift_coefficient = float(law["virtual_drag_coefficient"]), float(law["virtual_lift_coefficient"])
        s.tof_effective_distance = float(law["tof_effective_distance"])
        s.keep_distance, s.UWB_sensor_max_range = float(p.keep_distance), float(p.UWB_sensor_max_range)
        s.pid = self.pid_params()
        if target is not None:
            c, r = target_row(target)
            s.target[:] = [float(x) for x in c]
            s.target_radius = r
        return s

    def evaluate(self, p: Any, v: Any, q: Any, target: Any, pid_state: Any = None, pixel: Any = None):
        """fpv_chase_eval: the kernel's own lane function on the host, for n drones at once.  p [n, 3], v [n, 3], q [n, 4] (wxyz),
        `target` a Target or (centre, radius), `pid_state` [4, n] rows (integral, prev_derivative, previous_error, is_first; None: a
        freshly reset PID), `pixel` [n, 2] (x, y) or None = find the target.  Returns (rotation [n, 3, 3], thrust [n],
        pixel [n, 2], visible [n] bool, pid_state [4, n] after the call)."""
        pp, qq = poses(p, q)
        n = pp.shape[0]
        vv = np.ascontiguousarray(np.asarray(v, dtype=np.float32).reshape(n, 3))
        if pid_state is None:
            st = np.zeros((_lib.FPV_PID_ROWS, n), dtype=np.float32)
            st[3] = 1.0
        else:
            st = np.array(pid_state, dtype=np.float32, order="C").reshape(_lib.FPV_PID_ROWS, n)      # a[:, idx] is column-major
        s = self.derive(target)
        rot, thrust = np.zeros((n, 9), dtype=np.float32), np.zeros(n, dtype=np.float32)
        pix_out, vis = _aligned8(n), np.zeros(n, dtype=np.uint8)
        pix_in = None
        if pixel is not None:
            pix_in = _aligned8(n)
            pix_in[...] = np.asarray(pixel, dtype=np.float32).reshape(-1, 2)
            s.pixel = pix_in.ctypes.data
        s.pid_state, s.pid_ld = st.ctypes.data, n
        s.rotation, s.thrust, s.pixel_out, s.visible = rot.ctypes.data, thrust.ctypes.data, pix_out.ctypes.data, vis.ctypes.data
        _lib.check(_lib.lib().fpv_chase_eval(C.byref(s), n, pp.ctypes.data, vv.ctypes.data, qq.ctypes.data))
        return rot.reshape(n, 3, 3), thrust, np.array(pix_out), vis.astype(bool), st


def _aligned8(n: int) -> np.ndarray:
    """[n, 2] float32, 8-byte aligned"""
    buf = np.zeros(2 * n + 2, dtype=np.float32)
    off = (-buf.ctypes.data % 8) // 4
    return buf[off:off + 2 * n].reshape(n, 2)
