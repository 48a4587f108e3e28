"""The reference's guidance laws for N drones, one kernel each (include/fpv_abi.h "Target chase", "Point and shoot"), under the
reference's names.  A Racer batch has them too: the library refuses its handle by name."""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from . import _lib


class GuidanceLaws:
    """Mixed into `_Batch`.  The tensors are made by a law's first call - a batch that never calls one allocates none -, their names here."""
    force_multiplier_pid = None         # the guidance PID of a DroneBatch (a Racer has none: the laws then advance scratch rows)

    def _init_laws(self) -> None:
        self._chase_camera = self._chase_out = self._chase_track_out = self._chase_track_rows = self._chase_scratch_rows = None
        self._chase_structs, self._pns_structs, self._chase_keep, self._pns_out, self._pns_keep = {}, {}, None, None, None
        self.pns_prev_pixel = None      # [2, ld] Drone.prev_pixel of every drone (NaN = None), made by point and shoot's first use

    # -- target chase ------------------------------------------------------------------------------
    def _chase_rows(self) -> torch.Tensor:
        """The [4, ld] guidance-PID rows the law reads and advances: `force_multiplier_pid`'s own state where the batch has one"""
        pid = self.force_multiplier_pid
        if pid is not None:
            return pid.state
        if self._chase_scratch_rows is None:
            self._chase_scratch_rows = torch.zeros((_lib.FPV_PID_ROWS, self.ld), dtype=torch.float32, device=self.device)
        return self._chase_scratch_rows

    def set_chase_camera(self, camera=None, max_depth: float = 15.0) -> None:
        """The camera the target chase looks through - a fpyv_amd.camera.DepthCamera / Camera; None: the params' `camera` section,
        the reference's 640 x 480 - and the reach within which it sees the target (simulator.py:102: 15).  Takes effect with the
        next `calculate_needed_force_orientation` / `track` / `point_and_shoot`."""
        self._chase_camera, self._chase_structs, self._pns_structs = (camera, float(max_depth)), {}, {}

    def _chase(self, pixel, target, ref_frame: str, mode: str, rows: torch.Tensor):
        """One launch of fpv_chase_guide on torch's current stream into the preallocated outputs"""
        from .chase import ChaseGuidance, target_row
        if self._chase_camera is None:
            self.set_chase_camera()
        if self._chase_out is None:
            f32 = dict(dtype=torch.float32, device=self.device)
            self._chase_out = (torch.zeros((self.n, 3, 3), **f32), torch.zeros(self.n, **f32), torch.zeros((self.n, 2), **f32),
                               torch.zeros(self.n, dtype=torch.bool, device=self.device))
        key = (ref_frame, mode)
        if key not in self._chase_structs:
            camera, max_depth = self._chase_camera
            self._chase_structs[key] = ChaseGuidance(self.params, camera=camera, ref_frame=ref_frame, mode=mode, max_depth=max_depth).derive()
        s = self._chase_structs[key]
        c, r = target_row(target)
        s.target[:] = [float(x) for x in c]
        s.target_radius = r
        rot, thrust, pix, vis = self._chase_out
        if rows is not self._chase_rows():            # `track`: the law's outputs of a scratch PID go to scratch tensors
            if self._chase_track_out is None:
                self._chase_track_out = (torch.zeros_like(rot), torch.zeros_like(thrust))
            rot, thrust = self._chase_track_out
        keep = None
        if pixel is not None:
            keep = torch.as_tensor(np.asarray(pixel, dtype=np.float32) if not torch.is_tensor(pixel) else pixel,
                                   dtype=torch.float32, device=self.device)
            if keep.shape == (2,):
                keep = keep.expand(self.n, 2)
            if keep.shape != (self.n, 2):
                raise ValueError(f"pixel must be [2] or [{self.n}, 2] in (x, y) order, got {tuple(keep.shape)}")
            keep = keep.contiguous()
        s.pixel = keep.data_ptr() if keep is not None else None
        s.pid_state, s.pid_ld = rows.data_ptr(), rows.shape[1]
        s.rotation, s.thrust, s.pixel_out, s.visible = rot.data_ptr(), thrust.data_ptr(), pix.data_ptr(), vis.data_ptr()
        self._sensor_raw(self._L.fpv_chase_guide, s, None)
        self._chase_keep = keep
        return rot, thrust, pix, vis

    def calculate_needed_force_orientation(self, pixel, target, ref_frame: str = "world", mode: str = "level"):
        """Drone.calculate_needed_force_orientation (components.py:258-304) for every drone, one kernel: `pixel` [num_envs, 2]
        (x, y) where the drone's camera sees `target`, or None = find it (the projection of the target's centre; include/fpv_abi.h
        "Target chase").  Returns (rotation_matrix [num_envs, 3, 3], thrust_force [num_envs]) in preallocated tensors that the
        next call overwrites - what `step(..., rotation_matrix=, thrust_force=)` takes as they are.  A drone that does not see the
        target gets thrust_force NaN (step: not overridden) and an identity matrix.  Uses and advances `force_multiplier_pid`'s
        state for the drones it guides; `reset(mask)` clears it."""
        rot, thrust, _, _ = self._chase(pixel, target, ref_frame, mode, self._chase_rows())
        return rot, thrust

    def track(self, target):
        """(pixel [num_envs, 2] in (x, y) order, visible [num_envs] bool): where every drone's camera sees the centre of `target`
        (NaN where it does not) - the pixel alone: no PID is advanced and the outputs of the last
        `calculate_needed_force_orientation` stay as they are.  It is the same kernel run on scratch PID rows and scratch
        matrices: a launch of the whole law for its first step, not a kernel of its own."""
        if self._chase_track_rows is None:
            self._chase_track_rows = torch.zeros((_lib.FPV_PID_ROWS, self.ld), dtype=torch.float32, device=self.device)
        _, _, pix, vis = self._chase(None, target, "world", "level", self._chase_track_rows)
        return pix, vis

    # -- point and shoot ---------------------------------------------------------------------------
    @property
    def pns_pid_rows(self) -> Optional[torch.Tensor]:
        """The [4, ld] guidance-PID rows point and shoot advances (None before its first use): a checkpoint's rows"""
        return None if self.pns_prev_pixel is None else self._chase_rows()

    @property
    def pns_target_rows(self) -> Optional[torch.Tensor]:
        """The pursuit task's [3, ld] target positions where point and shoot is in use (else None): an env with assist= reads them
        BEFORE the step's pursuit call writes them again, so a checkpoint has to carry them"""
        return None if self.pns_prev_pixel is None else self.target_position_rows

    def _pns_rows(self) -> torch.Tensor:
        if self.pns_prev_pixel is None:
            self.pns_prev_pixel = torch.full((2, self.ld), float("nan"), dtype=torch.float32, device=self.device)
            f32 = dict(dtype=torch.float32, device=self.device)
            u8 = dict(dtype=torch.uint8, device=self.device)
            self._pns_out = dict(rotation=torch.zeros((self.n, 3, 3), **f32), thrust=torch.full((self.n,), float("nan"), **f32),
                                 pixel_velocity=torch.zeros((self.n, 2), **f32), limited=torch.zeros(self.n, **u8),
                                 visible=torch.zeros(self.n, **u8), throttle=torch.zeros(self.n, **f32))
        return self.pns_prev_pixel

    def _pns_struct(self, ref_frame: str, mode: str) -> "_lib.FpvPns":
        from .pns import PointAndShoot
        if self._chase_camera is None:
            self.set_chase_camera()
        key = (ref_frame, mode)
        if key not in self._pns_structs:
            camera, max_depth = self._chase_camera
            self._pns_structs[key] = PointAndShoot(self.params, camera=camera, ref_frame=ref_frame, mode=mode, max_depth=max_depth).derive()
        return self._pns_structs[key]

    def _pns_launch(self, s: "_lib.FpvPns", pixel, action, target, restart) -> None:
        """One launch of fpv_pns_guide on torch's current stream into the preallocated outputs: `pixel` None | [n, 2] tensor, `action`
        None | [n, 4] tensor, `target` None | host float32 [3] array | [3, >= n] device rows, `restart` None | [n] uint8 tensor"""
        prev, rows = self._pns_rows(), self._chase_rows()
        out = self._pns_out
        s.pid_state, s.pid_ld, s.prev_pixel, s.prev_pixel_ld = rows.data_ptr(), rows.shape[1], prev.data_ptr(), prev.shape[1]
        s.pixel = pixel.data_ptr() if pixel is not None else None
        s.action = action.data_ptr() if action is not None else None
        s.restart = restart.data_ptr() if restart is not None else None
        s.target = s.target_rows = None
        if isinstance(target, np.ndarray):
            s.target = target.ctypes.data
        elif target is not None:
            s.target_rows, s.target_ld = target.data_ptr(), target.stride(0)
        s.rotation, s.thrust, s.pixel_velocity = out["rotation"].data_ptr(), out["thrust"].data_ptr(), out["pixel_velocity"].data_ptr()
        s.limited, s.visible, s.throttle = out["limited"].data_ptr(), out["visible"].data_ptr(), out["throttle"].data_ptr()
        self._sensor_raw(self._L.fpv_pns_guide, s, None)
        self._pns_keep = (pixel, action, target, restart)

    def _per_drone(self, x, width: int, what: str) -> torch.Tensor:
        """[width] or [num_envs, width] -> contiguous float32 [num_envs, width] on the device"""
        t = torch.as_tensor(np.asarray(x, dtype=np.float32) if not torch.is_tensor(x) else x, dtype=torch.float32, device=self.device)
        if t.shape == (width,):
            t = t.expand(self.n, width)
        if t.shape != (self.n, width):
            raise ValueError(f"{what} must be [{width}] or [{self.n}, {width}], got {tuple(t.shape)}")
        return t.contiguous()

    def point_and_shoot(self, pixel, action, ref_frame: str = "world", mode: str = "level", target=None, restart=None):
        """Drone.point_and_shoot (components.py:312-381) for every drone, one kernel (include/fpv_abi.h "Point and shoot"): `pixel`
        [num_envs, 2] (x, y) where the drone's camera sees its target, or None = find it: then `target` is a Target or a centre [3]
        for all drones, or [3, >= num_envs] device rows with a centre per drone (`target_position_rows` of a pursuit task as they
        are).  `action` [4] or [num_envs, 4]: action[1] where on the image the target is to be held, action[2:] the virtual offset
        of the target in half-images (action[0] is not used: the reference discards what it feeds); None = zeros.  Returns
        (rotation_matrix [num_envs, 3, 3], thrust_force [num_envs]) in preallocated tensors that the next call overwrites - what
        `step(..., rotation_matrix=, thrust_force=)` takes as they are; `pixel_velocity`, `thrust_limited` and `pns_throttle` hold
        the call's other outputs.  A drone that does not see the target, or whose action is not finite, gets thrust_force NaN
        (step: not overridden) and an identity matrix.  The reference's thrust-limit loop is taken in closed form.
        Uses and advances `force_multiplier_pid`'s state and `pns_prev_pixel` for the drones it guides; `restart` [num_envs]
        flags drones that reset both first; `reset(mask)` clears them."""
        if ref_frame not in _lib.CHASE_FRAMES:
            raise ValueError("Unknown reference frame")                          # components.py:343
        if mode not in _lib.CHASE_MODES:
            raise ValueError("Unknown mode")                                     # components.py:377
        pix = None if pixel is None else self._per_drone(pixel, 2, "pixel")
        act = None if action is None else self._per_drone(action, 4, "action")
        tgt = None
        if target is not None:
            if torch.is_tensor(target) and target.dim() == 2:
                if target.shape[0] != 3 or target.shape[1] < self.n or target.stride(1) != 1 or target.dtype != torch.float32 or target.device != self._dev:
                    raise ValueError(f"target rows must be a float32 [3, >= {self.n}] tensor on {self.device} with unit column stride")
                tgt = target
            else:
                c = target.position if hasattr(target, "position") else target
                tgt = np.ascontiguousarray(np.asarray(c.cpu() if torch.is_tensor(c) else c, dtype=np.float32).reshape(3))
        elif pix is None:
            raise ValueError("pixel=None needs target=: a Target, a centre [3] or [3, num_envs] rows")
        rs = None
        if restart is not None:
            rs = torch.as_tensor(restart, device=self.device).to(torch.uint8).contiguous()
            if rs.shape != (self.n,):
                raise ValueError("restart must have shape (num_envs,)")
        self._pns_launch(self._pns_struct(ref_frame, mode), pix, act, tgt, rs)
        return self._pns_out["rotation"], self._pns_out["thrust"]

    @property
    def pixel_velocity(self) -> Optional[torch.Tensor]:
        """[num_envs, 2] Drone.pixel_velocity after the last `point_and_shoot`, pixels per second (NaN where the drone was not guided)"""
        return None if self.pns_prev_pixel is None else self._pns_out["pixel_velocity"]

    @property
    def thrust_limited(self) -> Optional[torch.Tensor]:
        """[num_envs] uint8 of the last `point_and_shoot`: 0 not limited, 1 thrust limit reached, 2 limit out of reach"""
        return None if self.pns_prev_pixel is None else self._pns_out["limited"]

    @property
    def pns_throttle(self) -> Optional[torch.Tensor]:
        """[num_envs] thrust2throttle(thrust_force) of the last `point_and_shoot`, in [-1, 1]"""
        return None if self.pns_prev_pixel is None else self._pns_out["throttle"]

    def _pns_reset(self, mask) -> None:
        """Drone.reset (components.py:166-168) for the law's rows: prev_pixel = None for the drones of `mask` (None = all)"""
        if self.pns_prev_pixel is None:
            return
        if mask is None:
            self.pns_prev_pixel.fill_(float("nan"))
        else:
            m = torch.as_tensor(mask, device=self.device).bool()
            self.pns_prev_pixel[:, :self.n].masked_fill_(m, float("nan"))
