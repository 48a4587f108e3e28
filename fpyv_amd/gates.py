"""Gate courses: the descriptor rows of a list of gates, a ready-made track, and the kernels' own gate function on the host.

A course is an ordered list of 1..64 `objects.Gate`s (or any object with the reference Gate's attributes `position`,
`rotation_matrix`, `size`, `shape`).  `DroneBatch(gates=course)` flies it: every drone has to pass the gates in order, the step
kernels detect the crossings and keep the per-drone race state (include/fpv_abi.h "Gate courses").
"""
from __future__ import annotations

import ctypes as C
from typing import Any, Optional, Sequence

import numpy as np

from . import _lib
from .objects import Gate


def _rows_of(gates: Sequence[Any]):
    arr = (_lib.FpvGate * max(1, len(gates)))()
    for k, g in enumerate(gates):
        if not hasattr(g, "as_gate_row"):            # e.g. the reference's own Gate
            g = Gate(g.position, g.rotation_matrix, g.size, getattr(g, "shape", "rectangle"))
        pos, rot, size, shape = g.as_gate_row()
        arr[k].position[:], arr[k].rotation[:], arr[k].size, arr[k].shape = pos, rot, size, shape
    return arr


def derive(gates: Sequence[Any]) -> np.ndarray:
    """[count, 16] float32 descriptor rows (c3 n3 u3 w3 a hz zc r2) by fpv_gates_derive - host arithmetic, no device.  Raises
    FpvError (FPV_EPARAM) naming the gate for a size that is not positive, a rotation that is not orthonormal to 1e-6, an
    unknown shape code, or a count outside 1..64."""
    gates = list(gates)
    out = np.zeros((max(1, len(gates)), _lib.FPV_GATE_FLOATS), dtype=np.float32)
    arr = _rows_of(gates)
    _lib.check(_lib.lib().fpv_gates_derive(len(gates), C.addressof(arr), out.ctypes.data))
    return out


def yaw_matrix(yaw: float) -> np.ndarray:
    c, s = np.cos(yaw), np.sin(yaw)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def circular_track(count: int, radius: float, gate_size: float, height: float = 0.0, shapes=("rectangle", "circle", "half_circle")):
    """`count` gates on a circle of `radius` around the z axis at `height`, flown counter-clockwise: gate k stands at angle
    2 pi k / count with its normal along the tangent of the circle, shapes cycling through `shapes`.  (Our own formulation of a
    round track; the reference's generate_track places and sizes its gates differently.)"""
    if count < 1 or count > _lib.FPV_MAX_GATES:
        raise ValueError(f"a course has 1..{_lib.FPV_MAX_GATES} gates")
    out = []
    for k in range(count):
        th = 2.0 * np.pi * k / count
        pos = np.array([radius * np.cos(th), radius * np.sin(th), height])
        out.append(Gate(pos, yaw_matrix(th + np.pi / 2), gate_size, shape=shapes[k % len(shapes)]))
    return out


def evaluate(rows: np.ndarray, p_old, p_new, q_new, physics_done, word_in, laps: int = 0, gate_rewards=None,
             miss_is_done: bool = False, gate_start=None, auto_reset: bool = False, p_after=None, q_after=None):
    """fpv_gate_eval: the step kernels' own gate function on the host, for n drones at once.  `rows` [count, 16] float32
    (`derive`), p_old / p_new [n, 3], q_new [n, 4] (wxyz), physics_done [n], word_in [n] uint32.  Returns (word_out [n] uint32,
    reward [n] float32, done [n] bool, obs [n, 6] float32)."""
    f32 = lambda a, w: np.ascontiguousarray(np.asarray(a, dtype=np.float32).reshape(-1, w))  # noqa: E731
    rows = np.ascontiguousarray(rows, dtype=np.float32).reshape(-1, _lib.FPV_GATE_FLOATS)
    po, pn, qn = f32(p_old, 3), f32(p_new, 3), f32(q_new, 4)
    n = po.shape[0]
    pd = np.ascontiguousarray(np.asarray(physics_done).reshape(-1).astype(np.uint8))
    wi = np.ascontiguousarray(np.asarray(word_in).reshape(-1).astype(np.uint32))
    if not (pn.shape[0] == qn.shape[0] == pd.shape[0] == wi.shape[0] == n):
        raise ValueError("p_old, p_new, q_new, physics_done and word_in must describe the same n drones")
    c = _lib.pack_course(rows.shape[0], laps, gate_rewards, miss_is_done)
    c.descriptors = rows.ctypes.data
    st = None
    if gate_start is not None:
        st = np.ascontiguousarray(np.asarray(gate_start).reshape(-1).astype(np.uint8))
        if st.shape[0] != n:
            raise ValueError("gate_start must have n entries")
        c.gate_start = st.ctypes.data
    pa = None if p_after is None else f32(p_after, 3)
    qa = None if q_after is None else f32(q_after, 4)
    wo, rew = np.zeros(n, np.uint32), np.zeros(n, np.float32)
    dn, obs = np.zeros(n, np.uint8), np.zeros((n, 6), np.float32)
    ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    _lib.check(_lib.lib().fpv_gate_eval(C.byref(c), n, po.ctypes.data, pn.ctypes.data, qn.ctypes.data, pd.ctypes.data, wi.ctypes.data,
                                        int(bool(auto_reset)), ptr(pa), ptr(qa), wo.ctypes.data, rew.ctypes.data, dn.ctypes.data,
                                        obs.ctypes.data))
    return wo, rew, dn.astype(bool), obs


def word_fields(word):
    """(next gate, event, gates passed) of gate words (NumPy array or torch tensor of any integer dtype)"""
    return word & 0xFF, (word >> 8) & 3, (word >> 10) & 0x3FFFFF
