"""Point and shoot: the reference's steered guidance law `Drone.point_and_shoot(pixel, action, ref_frame, mode)`
(/root/reference/src/utils/components.py:312-381) for N drones, and the kernel's own lane function on the host.

`PointAndShoot` holds what the law reads besides the drones: the camera, the three constants of params.yaml's `point_and_shoot`
section, the mass, the guidance PID's constants, the thrust limit `max_throttle_in_force`, the inverse thrust polynomial of
`thrust2throttle`, the frame and the mode.  `DroneBatch.point_and_shoot(pixel, action)` runs the law in one kernel and returns
tensors that go straight back into `batch.step(..., rotation_matrix=, thrust_force=)`; `FpvVecEnv(pursuit=, assist=PointAndShoot(..))`
makes the law's four commands the environment's action (include/fpv_abi.h "Point and shoot").
"""
from __future__ import annotations

import ctypes as C
from typing import Any, Optional

import numpy as np

from . import _lib
from .camera import DepthCamera
from .chase import ChaseGuidance, _aligned8
from .rays import poses


class PointAndShoot(ChaseGuidance):
    """The law's uniform inputs.  `params` is a DroneParams; `camera` a DepthCamera / Camera replacing the params' own; `ref_frame`
    "world" | "drone" and `mode` "level" | "frontarget" default to `params.point_and_shoot`'s; `max_depth` is the reach within which
    a target's centre is seen when no pixel is given."""

    def __init__(self, params: Any, camera: Optional[DepthCamera] = None, ref_frame: Optional[str] = None, mode: Optional[str] = None,
                 max_depth: float = 15.0):
        law = params.point_and_shoot
        super().__init__(params, camera=camera, ref_frame=law.get("ref_frame", "world") if ref_frame is None else ref_frame,
                         mode=law.get("mode", "level") if mode is None else mode, max_depth=max_depth)

    def derive(self) -> "_lib.FpvPns":                                         # pylint: disable=arguments-differ
        """A fresh fpv_pns_t holding the camera numbers (fpv_chase_derive's), the constants, the frame and the mode; the pointers
        are the caller's to fill - host arithmetic, no device.  Raises FpvError naming what it refuses."""
        c = super().derive()
        s = _lib.FpvPns()
        s.struct_size = C.sizeof(_lib.FpvPns)
        for f in ("width", "height", "ref_frame", "mode", "focal_length", "relative_rotation", "relative_position", "max_depth", "mass",
                  "virtual_drag_coefficient", "virtual_lift_coefficient", "tof_effective_distance", "pid"):
            setattr(s, f, getattr(c, f))
        s.max_throttle_in_force = float(self.params.max_throttle_in_force)
        s.thrust2throttle_poly[:] = [float(x) for x in self.params.thrust2throttle_poly]
        return s

    def evaluate(self, p: Any, v: Any, q: Any, pixel: Any = None, action: Any = None, target: Any = None, pid_state: Any = None,
                 prev_pixel: Any = None, restart: Any = None) -> dict:               # pylint: disable=arguments-differ
        """fpv_pns_eval: the kernel's own lane function on the host, for n drones at once.  p [n, 3], v [n, 3], q [n, 4] (wxyz);
        `pixel` [n, 2] (x, y) or None = project `target` ([3] one for all, or [3, n] rows); `action` [4] | [n, 4] | None = zeros;
        `pid_state` [4, n] rows (None: a freshly reset PID), `prev_pixel` [2, n] (None: NaN, the first call), `restart` [n] or None.
        Returns a dict: rotation [n, 3, 3], thrust [n], throttle [n], pixel_velocity [n, 2], limited [n] uint8, visible [n] bool,
        pid_state [4, n] and prev_pixel [2, n] after the call."""
        pp, qq = poses(p, q)
        n = pp.shape[0]
        vv = np.ascontiguousarray(np.asarray(v, dtype=np.float32).reshape(n, 3))
        if pid_state is None:
            st = np.zeros((_lib.FPV_PID_ROWS, n), dtype=np.float32)
            st[3] = 1.0
        else:
            st = np.array(pid_state, dtype=np.float32, order="C").reshape(_lib.FPV_PID_ROWS, n)
        prev = np.full((2, n), np.nan, dtype=np.float32) if prev_pixel is None else np.array(prev_pixel, dtype=np.float32, order="C").reshape(2, n)
        s = self.derive()
        keep = []
        if pixel is not None:
            pix_in = _aligned8(n)
            pix_in[...] = np.asarray(pixel, dtype=np.float32).reshape(-1, 2)
            s.pixel = pix_in.ctypes.data
            keep.append(pix_in)
        if target is not None:
            t = np.ascontiguousarray(np.asarray(getattr(target, "position", target), dtype=np.float32))
            if t.shape == (3,):
                s.target = t.ctypes.data
            elif t.shape == (3, n):
                s.target_rows, s.target_ld = t.ctypes.data, n
            else:
                raise ValueError(f"target must be [3] or [3, {n}] rows, got {t.shape}")
            keep.append(t)
        if action is not None:
            a = np.broadcast_to(np.asarray(action, dtype=np.float32), (n, 4))
            act = _aligned16(n)
            act[...] = a
            s.action = act.ctypes.data
            keep.append(act)
        if restart is not None:
            rs = np.ascontiguousarray(np.asarray(restart).astype(np.uint8).reshape(n))
            s.restart = rs.ctypes.data
            keep.append(rs)
        rot, thrust, throttle = np.zeros((n, 9), dtype=np.float32), np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.float32)
        vel, lim, vis = _aligned8(n), np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8)
        s.pid_state, s.pid_ld, s.prev_pixel, s.prev_pixel_ld = st.ctypes.data, n, prev.ctypes.data, n
        s.rotation, s.thrust, s.throttle = rot.ctypes.data, thrust.ctypes.data, throttle.ctypes.data
        s.pixel_velocity, s.limited, s.visible = vel.ctypes.data, lim.ctypes.data, vis.ctypes.data
        _lib.check(_lib.lib().fpv_pns_eval(C.byref(s), n, pp.ctypes.data, vv.ctypes.data, qq.ctypes.data))
        return dict(rotation=rot.reshape(n, 3, 3), thrust=thrust, throttle=throttle, pixel_velocity=np.array(vel), limited=lim,
                    visible=vis.astype(bool), pid_state=st, prev_pixel=prev)


def _aligned16(n: int) -> np.ndarray:
    """[n, 4] float32, 16-byte aligned"""
    buf = np.zeros(4 * n + 4, dtype=np.float32)
    off = (-buf.ctypes.data % 16) // 4
    return buf[off:off + 4 * n].reshape(n, 4)
