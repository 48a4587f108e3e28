"""Pursuit task: the reference's chase scenario (/root/reference/src/core/simulator.py:54-110) for N drones - every drone has a
`Target` of its own on a circular path of its own, the targets are advanced on the device, the distance pays a reward, a capture
respawns the target, the target is observed in the body frame and, optionally, the reference's guidance law runs against each
drone's own target in the same launch (include/fpv_abi.h "Pursuit task").

`PursuitTask` holds what a call reads besides the drones and their target rows; `DroneBatch(..., pursuit=task)` and
`FpvVecEnv(pursuit=task)` allocate the rows and launch the kernel after every reset and step.  `evaluate` is the kernel's own lane
function on the host (fpv_pursuit_eval): the same bits.
"""
from __future__ import annotations

import ctypes as C
from typing import Any, Dict, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from .objects import Target
from .rays import poses

ROWS = _lib.FPV_TGT_ROWS
DEFAULT_PATH = dict(radius=25.0, resolution=5500)               # config/params.yaml simulator.targets.path


def generate_targets(count: int, center: Sequence[float], std: float, size: float, variation: float, nu: Any = None,
                     path: Optional[Dict[str, Any]] = None, seed: int = 0):
    """The reference's factory (generators.py:21-24) with a generator of its own: the draws `np.random.seed(seed)` followed by the
    reference's call would make, in its order (three normals for the centre, one for the size, per target)."""
    rng = np.random.RandomState(seed)
    return [Target(np.array(center, dtype=np.float64) + std * rng.randn(3), np.abs(size + variation * rng.randn()), nu, path)
            for _ in range(count)]


def targets_from_params(section: Dict[str, Any], seed: int = 0):
    """`generate_targets(**params["simulator"]["targets"])` (simulator.py:54): count, center, std, size, variation, nu, path"""
    return generate_targets(seed=seed, **section)


def aligned(shape: Tuple[int, ...], dtype: Any = np.float32, align: int = 16) -> np.ndarray:
    """zeros of `shape` whose first byte is `align`-byte aligned"""
    count, item = int(np.prod(shape)), np.dtype(dtype).itemsize
    raw = np.zeros(count * item + align, dtype=np.uint8)
    off = -raw.ctypes.data % align
    return raw[off:off + count * item].view(dtype).reshape(shape)


def circle_table(resolution: int) -> np.ndarray:
    """fpv_pursuit_derive: [K, 2] float32 (cos, sin) of the reference's path angles, 8-byte aligned"""
    k = int(resolution)
    out = aligned((max(k, 1), 2), np.float32, 8)
    _lib.check(_lib.lib().fpv_pursuit_derive(k, out.ctypes.data))
    return out


class PursuitTask:
    """targets: a list of fpyv_amd.objects.Target (or anything with `.position` / `.center`, `.radius` and optionally `.path`), one
         per drone or one for all - a Target that was update()d k times continues from there, one with path=None stands still -;
         or a dict of arrays centre [n | 1, 3], radius, path_radius, phase; None: the reference's default target at (0, 0, 3)
       path: dict(radius=, resolution=), the reference's 25 m / 5500 by default - the resolution K is shared by all (one table);
         the radius is that of a dict of arrays that names none
       rewards: dict(progress=, capture=); respawn: dict(lo=[3], hi=[3], radius=(lo, hi), seed=)
       guide: None | dict(ref_frame=, mode=, camera=, max_depth=) - the target chase's law against each drone's own target"""

    def __init__(self, targets: Any = None, path: Optional[Dict[str, Any]] = None, capture_distance: float = 0.0,
                 rewards: Optional[Dict[str, float]] = None, respawn: Optional[Dict[str, Any]] = None, respawn_on_done: bool = True,
                 obs: bool = True, guide: Optional[Dict[str, Any]] = None, add_to_reward: bool = True):
        self.path = {**DEFAULT_PATH, **(path or {})}
        self.resolution = int(self.path["resolution"])
        self.targets = targets if targets is not None else dict(centre=[0.0, 0.0, 3.0], radius=1.0)
        self.capture_distance = float(capture_distance)
        rw = dict(rewards or {})
        self.progress, self.capture = float(rw.pop("progress", 1.0)), float(rw.pop("capture", 10.0))
        if rw:
            raise ValueError(f"unknown reward(s) {sorted(rw)}: progress, capture")
        rs = dict(respawn or {})
        self.spawn_lo = [float(x) for x in rs.pop("lo", (-10.0, -10.0, 1.0))]
        self.spawn_hi = [float(x) for x in rs.pop("hi", (10.0, 10.0, 6.0))]
        self.radius_lo, self.radius_hi = (float(x) for x in rs.pop("radius", (0.5, 1.0)))
        self.spawn_seed = int(rs.pop("seed", 0)) & 0xFFFFFFFFFFFFFFFF
        if rs:
            raise ValueError(f"unknown respawn key(s) {sorted(rs)}: lo, hi, radius, seed")
        self.respawn_on_done, self.obs, self.add_to_reward = bool(respawn_on_done), bool(obs), bool(add_to_reward)
        if guide is not None:
            bad = set(guide) - {"ref_frame", "mode", "camera", "max_depth"}
            if bad:
                raise ValueError(f"unknown guide key(s) {sorted(bad)}: ref_frame, mode, camera, max_depth")
        self.guide = dict(guide) if guide is not None else None
        self._circle = None

    # -- the tables -------------------------------------------------------------------------------------------------------------
    @property
    def circle(self) -> np.ndarray:
        if self._circle is None:
            self._circle = circle_table(self.resolution)
        return self._circle

    def rows(self, n: int, ld: Optional[int] = None, targets: Any = None) -> np.ndarray:
        """The target rows [8, ld] float32 (words bit-cast) of `targets` (None: the task's) for n drones, freshly set: PREV_DIST 0,
        COUNT = phase | FRESH, SPAWNS 0.  16-byte aligned; ld defaults to n rounded up to 4."""
        ld = int(ld) if ld is not None else (n + 3) // 4 * 4
        t = self.targets if targets is None else targets
        if isinstance(t, dict):
            centre = np.broadcast_to(np.asarray(t["centre"], dtype=np.float32).reshape(-1, 3), (n, 3))
            radius = np.broadcast_to(np.asarray(t.get("radius", 1.0), dtype=np.float32).reshape(-1), (n,))
            path_r = np.broadcast_to(np.asarray(t.get("path_radius", self.path["radius"]), dtype=np.float32).reshape(-1), (n,))
            phase = np.broadcast_to(np.asarray(t.get("phase", 0), dtype=np.int64).reshape(-1), (n,))
        else:
            t = list(t) if isinstance(t, (list, tuple)) else [t]
            if len(t) not in (1, n):
                raise ValueError(f"{len(t)} targets for {n} drones: one per drone, or one for all")
            t = t * n if len(t) == 1 else t
            centre = np.array([np.asarray(getattr(x, "center", x.position), dtype=np.float32).reshape(3) for x in t], dtype=np.float32)
            radius = np.array([getattr(x, "radius", 0.0) for x in t], dtype=np.float32)
            paths = [getattr(x, "path", None) for x in t]
            for p in paths:
                if isinstance(p, dict) and int(p.get("resolution", self.resolution)) != self.resolution:
                    raise ValueError(f"a target's path resolution {p['resolution']} is not the task's {self.resolution}: the table is shared")
            path_r = np.array([float(p["radius"]) if isinstance(p, dict) else 0.0 for p in paths], dtype=np.float32)
            phase = np.array([int(getattr(x, "_count", 0)) % self.resolution for x in t], dtype=np.int64)
        if np.any(phase < 0) or np.any(phase >= self.resolution):
            raise ValueError(f"a phase must be a path index in [0, {self.resolution})")
        out = aligned((ROWS, ld), np.float32, 16)
        out[_lib.TGT_CX:_lib.TGT_CZ + 1, :n] = centre.T
        out[_lib.TGT_PATH_R, :n], out[_lib.TGT_RADIUS, :n] = path_r, radius
        out.view(np.uint32)[_lib.TGT_COUNT, :n] = phase.astype(np.uint32) | np.uint32(_lib.FPV_TGT_FRESH)
        return out

    def chase(self, params: Any) -> Optional["_lib.FpvChase"]:
        """the guidance law's fpv_chase_t (fpyv_amd.chase.ChaseGuidance.derive) or None; the pointers are the caller's to fill"""
        if self.guide is None:
            return None
        from .chase import ChaseGuidance
        g = self.guide
        return ChaseGuidance(params, camera=g.get("camera"), ref_frame=g.get("ref_frame", "world"), mode=g.get("mode", "level"),
                             max_depth=g.get("max_depth", 15.0)).derive()

    def derive(self, dt: float, advance: bool = True) -> "_lib.FpvPursuit":
        """A fresh fpv_pursuit_t holding the constants, the flags and the table (the other pointers are the caller's to fill; the
        struct keeps the table alive) - host arithmetic, no device."""
        s = _lib.FpvPursuit()
        s.struct_size = C.sizeof(_lib.FpvPursuit)
        s.path_resolution, s.advance, s.respawn_on_done, s.add_to_reward = self.resolution, int(advance), int(self.respawn_on_done), int(self.add_to_reward)
        s.spawn_seed, s.dt, s.capture_distance, s.progress, s.capture = self.spawn_seed, float(dt), self.capture_distance, self.progress, self.capture
        s.spawn_lo[:], s.spawn_hi[:] = self.spawn_lo, self.spawn_hi
        s.radius_lo, s.radius_hi = self.radius_lo, self.radius_hi
        s._circle_keep = self.circle
        s.circle = self.circle.ctypes.data
        return s

    def sample(self, global_id: int, respawn_index: int) -> Tuple[np.ndarray, float, int]:
        """fpv_pursuit_sample: (centre [3] float32, radius, phase) of drone `global_id`'s respawn number `respawn_index`"""
        s = self.derive(1.0)
        out, phase = np.zeros(4, dtype=np.float32), C.c_uint32()
        _lib.check(_lib.lib().fpv_pursuit_sample(C.byref(s), int(global_id), int(respawn_index), out.ctypes.data, C.byref(phase)))
        return out[:3].copy(), float(out[3]), int(phase.value)

    def evaluate(self, p: Any, v: Any, q: Any, rows: np.ndarray, dt: float, done: Any = None, reward: Any = None, reset: bool = False,
                 advance: bool = True, drone_id_offset: int = 0, pid_state: Any = None, params: Any = None) -> Dict[str, np.ndarray]:
        """fpv_pursuit_eval: the kernel's own lane function on the host, for n drones at once.  p [n, 3], v [n, 3], q [n, 4] (wxyz);
        `rows` [8, >= n] the target rows BEFORE the call (not modified); `done` [n] the done bytes - or, with reset=True, the mask
        (None = all); `reward` [n] the step's reward (add_to_reward adds to a copy).  With `guide`, `params` is the DroneParams and
        `pid_state` [4, n] the guidance PID rows (None: freshly reset).  Returns a dict: rows (after), obs [7, n], position [3, n],
        event [n], paid [n], reward [n] and, with `guide`, rotation [n, 3, 3], thrust [n], pixel [n, 2], visible [n], pid_state."""
        pp, qq = poses(p, q)
        n = pp.shape[0]
        vv = np.ascontiguousarray(np.asarray(v, dtype=np.float32).reshape(n, 3))
        ld = (n + 3) // 4 * 4
        t = aligned((ROWS, ld), np.float32, 16)
        t[:, :n] = np.asarray(rows, dtype=np.float32)[:, :n]
        s = self.derive(dt, advance)
        obs, pos = np.zeros((_lib.FPV_PURSUIT_OBS, n), dtype=np.float32), np.zeros((3, n), dtype=np.float32)
        event, paid = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.float32)
        rew = np.zeros(n, dtype=np.float32) if reward is None else np.array(reward, dtype=np.float32).reshape(n)
        flags = None if done is None else np.ascontiguousarray(np.asarray(done).astype(np.uint8).reshape(n))
        s.targets, s.targets_ld = t.ctypes.data, ld
        s.obs, s.obs_ld, s.position, s.position_ld = obs.ctypes.data, n, pos.ctypes.data, n
        s.event, s.reward_out = event.ctypes.data, paid.ctypes.data
        out = dict(rows=t, obs=obs, position=pos, event=event, paid=paid, reward=rew)
        g = self.chase(params)
        if g is not None:
            from .chase import _aligned8
            if pid_state is None:
                st = np.zeros((_lib.FPV_PID_ROWS, n), dtype=np.float32)
                st[_lib_pid_first()] = 1.0
            else:
                st = np.array(pid_state, dtype=np.float32, order="C").reshape(_lib.FPV_PID_ROWS, n)
            rot, thrust, pix, vis = np.zeros((n, 9), dtype=np.float32), np.zeros(n, dtype=np.float32), _aligned8(n), np.zeros(n, dtype=np.uint8)
            g.pid_state, g.pid_ld, g.rotation, g.thrust = st.ctypes.data, n, rot.ctypes.data, thrust.ctypes.data
            g.pixel_out, g.visible = pix.ctypes.data, vis.ctypes.data
            s.guide = C.pointer(g)
            out.update(rotation=rot.reshape(n, 3, 3), thrust=thrust, pixel=pix, visible=vis, pid_state=st)
        _lib.check(_lib.lib().fpv_pursuit_eval(C.byref(s), n, int(drone_id_offset), pp.ctypes.data, vv.ctypes.data, qq.ctypes.data,
                                               None if flags is None else flags.ctypes.data, rew.ctypes.data, int(bool(reset))))
        if g is not None:
            out["visible"] = out["visible"].astype(bool)
            out["pixel"] = np.array(out["pixel"])
        return out


def _lib_pid_first() -> int:
    return 3            # FPV_PID_IS_FIRST


def captures(rows: Any):
    """captures in the current episode, per drone, of target rows (NumPy [8, n] float32 or a torch tensor of them)"""
    if isinstance(rows, np.ndarray):
        return rows.view(np.uint32)[_lib.TGT_SPAWNS] >> 16
    import torch
    return (rows[_lib.TGT_SPAWNS].view(torch.int32) >> 16) & 0xFFFF
