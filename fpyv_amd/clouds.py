"""Point clouds of the world objects: what the reference's camera renders (include/fpv_abi.h "Point-cloud camera").

The deterministic generators of the reference, restated (nothing is copied) - the formulas are computed by `fpv_cloud_derive`
(csrc/fpv_splat.h fpv_cloud_points) in double and narrowed once to float32:

    Ground    the resolution^2 grid at z = 0                       src/utils/components.py:655-664, random=False
    Cylinder  the angle_resolution x height_resolution mesh + position                       components.py:697-708, random=False
    Gate      the corner points at its resolution and the first corner again                 components.py:790-805
    Target    vertices * radius + position                                                   components.py:758-771

A `random=True` Ground or Cylinder has no cloud here: pass its points as a raw object (anything with a `.points` [P, 3] array).  The
default vertices of a Target are this build's own icosphere (`icosphere(nu)`: 10 nu^2 + 2 unit vertices); the `icosphere` package the
reference imports is not a dependency, and the agreement of the two vertex sets is NOT checked - `Target(..., vertices=)` takes the
unit vertices of your choice.

`PointCloud.from_world(object_list, gates=())` flattens a world into what `fpv_splat_t` takes: float32 points as SoA [3, point_ld],
`first` [M + 1], a translation `offset` [M, 3] per object (zero but for Targets, whose local vertices stay put while `Target.update()`
moves the offset) and the local `box` [M, 6] of every object - the min and max of its points, which is what the reference's
`helper_functions.bbox3d` computes.
"""
from __future__ import annotations

import ctypes as C
from typing import Any, List, Sequence

import numpy as np

from . import _lib


def _derive(kind: int, numbers: Sequence[float], resolutions: Sequence[int]) -> np.ndarray:
    """fpv_cloud_derive -> [P, 3] float32"""
    num = (C.c_double * len(numbers))(*[float(x) for x in numbers])
    res = (C.c_int32 * len(resolutions))(*[int(x) for x in resolutions])
    L = _lib.lib()
    count = L.fpv_cloud_derive(kind, C.addressof(num), C.addressof(res), None, 0)
    if count < 0:
        _lib.check(count)
    ld = max(4, (count + 3) // 4 * 4)
    out = np.zeros((3, ld), dtype=np.float32)
    rc = L.fpv_cloud_derive(kind, C.addressof(num), C.addressof(res), out.ctypes.data, ld)
    if rc < 0:
        _lib.check(rc)
    return np.ascontiguousarray(out[:, :count].T)


def ground_points(size: float, resolution: int) -> np.ndarray:
    """[resolution^2, 3] float32: the grid of components.py:662-664 (x fastest); no points below resolution 1"""
    if int(resolution) < 1:
        return np.zeros((0, 3), dtype=np.float32)
    return _derive(_lib.CLOUD_GROUND, [size], [resolution])


def cylinder_points(position: Sequence[float], radius: float, height: float, angle_resolution: int, height_resolution: int) -> np.ndarray:
    """[angle_resolution * height_resolution, 3] float32: the mesh of components.py:702-707 (angle fastest) plus the position"""
    if int(angle_resolution) < 1 or int(height_resolution) < 1:
        return np.zeros((0, 3), dtype=np.float32)
    p = np.asarray(position, dtype=np.float64).reshape(3)
    return _derive(_lib.CLOUD_CYLINDER, [p[0], p[1], p[2], radius, height], [angle_resolution, height_resolution])


def gate_points(position: Sequence[float], rotation_matrix: Any, size: float, shape_code: int, resolution: int = 17) -> np.ndarray:
    """[corners + 1, 3] float32: the corner points of components.py:790-805, the first one repeated"""
    p = np.asarray(position, dtype=np.float64).reshape(3)
    R = np.asarray(rotation_matrix, dtype=np.float64).reshape(9)
    return _derive(_lib.CLOUD_GATE, [*p, *R, size], [shape_code, resolution])


def icosphere(nu: int = 1) -> np.ndarray:
    """[10 nu^2 + 2, 3] float64 unit vertices: every face of the icosahedron cut into nu^2 triangles, the grid points pushed out to the
    sphere.  This build's own; its vertex order and, for nu > 1, its vertex positions are not held to the `icosphere` package's."""
    nu = int(nu)
    if nu < 1:
        raise ValueError("nu must be >= 1")
    t = (1.0 + np.sqrt(5.0)) / 2.0
    v = np.array([[-1, t, 0], [1, t, 0], [-1, -t, 0], [1, -t, 0], [0, -1, t], [0, 1, t], [0, -1, -t], [0, 1, -t],
                  [t, 0, -1], [t, 0, 1], [-t, 0, -1], [-t, 0, 1]], dtype=np.float64)
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    faces = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
             (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    out, seen = [], set()
    for a, b, c in faces:
        for i in range(nu + 1):
            for j in range(nu + 1 - i):
                x = (v[a] * (nu - i - j) + v[b] * i + v[c] * j) / nu
                x = x / np.linalg.norm(x)
                key = tuple(np.round(x * 1e6).astype(np.int64).tolist())
                if key not in seen:
                    seen.add(key)
                    out.append(x)
    return np.array(out, dtype=np.float64)


def _is_target(o: Any) -> bool:
    return type(o).__name__ == "Target" and hasattr(o, "vertices") and hasattr(o, "position")


class PointCloud:
    """The clouds of a world, flattened (see the module).  `points` [3, point_ld] float32, `first` [M + 1] int32, `offset` [M, 3]
    float32, `box` [M, 6] float32, `count` = M, `total` = first[M].  `refresh()` re-reads the positions of the Targets into `offset`."""

    def __init__(self, clouds: Sequence[np.ndarray], offsets: Any = None, movers: Sequence[Any] = ()):
        clouds = [np.asarray(c, dtype=np.float32).reshape(-1, 3) for c in clouds]
        m = len(clouds)
        if m > _lib.FPV_MAX_BOXES:
            raise ValueError(f"a point cloud has at most {_lib.FPV_MAX_BOXES} objects, not {m}")
        sizes = [c.shape[0] for c in clouds]
        self.first = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        self.count, self.total = m, int(self.first[-1])
        if self.total > _lib.FPV_SPLAT_MAX_POINTS:
            raise ValueError(f"a point cloud has at most 2^20 points, not {self.total}")
        self.first = self.first.astype(np.int32)
        self.point_ld = max(4, (self.total + 3) // 4 * 4)
        self.points = np.zeros((3, self.point_ld), dtype=np.float32)
        self.box = np.zeros((m, 6), dtype=np.float32)
        for k, c in enumerate(clouds):
            self.points[:, self.first[k]:self.first[k + 1]] = c.T
            if c.shape[0]:
                self.box[k, :3], self.box[k, 3:] = c.min(axis=0), c.max(axis=0)
        self.offset = np.zeros((m, 3), dtype=np.float32)
        if offsets is not None:
            self.offset[...] = np.asarray(offsets, dtype=np.float32).reshape(m, 3)
        self._movers = list(movers)                       # (slot, object): the Targets, whose position is the offset

    @classmethod
    def from_world(cls, object_list: Sequence[Any] = (), gates: Sequence[Any] = ()) -> "PointCloud":
        """Every entry of `object_list` that has a `.points` array - this package's objects, the reference's own, raw ones - in list
        order, then `gates`; Trails are skipped.  A Target (an object of a class named so, with `vertices` and `position`) keeps its
        local vertices as points and its position as the offset."""
        clouds: List[np.ndarray] = []
        offsets: List[Any] = []
        movers = []
        for o in list(object_list or ()) + list(gates or ()):
            if type(o).__name__ == "Trail":
                continue
            if _is_target(o):
                movers.append((len(clouds), o))
                clouds.append(np.asarray(o.vertices, dtype=np.float64))
                offsets.append(np.asarray(o.position, dtype=np.float64).reshape(3))
            else:
                pts = getattr(o, "points", None)
                if pts is None:
                    raise ValueError(f"{type(o).__name__} has no points: a cloud takes objects with a .points [P, 3] array")
                clouds.append(np.asarray(pts, dtype=np.float64).reshape(-1, 3))
                offsets.append(np.zeros(3))
        return cls(clouds, np.array(offsets).reshape(len(clouds), 3), movers)

    def refresh(self) -> bool:
        """The Targets' positions as they are now into `offset`; True when one moved"""
        moved = False
        for k, o in self._movers:
            new = np.asarray(o.position, dtype=np.float32).reshape(3)
            if not np.array_equal(new, self.offset[k]):
                self.offset[k], moved = new, True
        return moved

    def world_points(self, k: int) -> np.ndarray:
        """[P, 3] float32: the points of object k where they are (points + offset, in float32 like the kernel)"""
        return self.points[:, self.first[k]:self.first[k + 1]].T + self.offset[k]

    def fill(self, s: "_lib.FpvSplat") -> None:
        """object_count, first, offset and box of `s` (the by-value tables); the points pointer is the caller's"""
        s.object_count = self.count
        C.memmove(s.first, self.first.ctypes.data, 4 * (self.count + 1))
        if self.count:
            C.memmove(s.offset, np.ascontiguousarray(self.offset).ctypes.data, 12 * self.count)
            C.memmove(s.box, np.ascontiguousarray(self.box).ctypes.data, 24 * self.count)
        s.point_ld = self.point_ld
