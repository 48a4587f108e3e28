"""Per-drone physics on the host side of the boundary (include/fpv_abi.h "Per-drone physics"): parameter sets as
[n, FPV_PHYS_INPUTS] float64 arrays - mass, c3 c2 c1 c0, Cd x y z, rates_transition_rate, thrust_transition_rate -, their
table columns through fpv_physics_derive and random draws through fpv_physics_sample.  Host arithmetic in the C library; nothing
here touches the GPU (DroneBatch.set_physics / randomize_physics upload the result).
"""
from __future__ import annotations

import ctypes as C
from typing import Any, Optional, Sequence

import numpy as np

from . import _lib

ROWS, INPUTS = _lib.FPV_PHYS_ROWS, _lib.FPV_PHYS_INPUTS


def base_inputs(cp: _lib.FpvParams) -> np.ndarray:
    """[FPV_PHYS_INPUTS] float64: the parameter set of the base parameters themselves"""
    return np.array([cp.mass, *cp.thrust_poly, *cp.drag_coefficients, cp.rates_transition_rate, cp.thrust_transition_rate],
                    dtype=np.float64)


def _cols(x: Any, n: int, k: int, name: str) -> np.ndarray:
    a = np.asarray(x, dtype=np.float64)
    if a.ndim == 1 and k == 1 and a.shape[0] == n:
        a = a[:, None]
    try:
        return np.broadcast_to(a, (n, k))
    except ValueError:
        raise ValueError(f"{name} must be a scalar, [{n}]" + (f", [{k}] or [{n}, {k}]" if k > 1 else "") + f", got {a.shape}") from None


def inputs(cp: _lib.FpvParams, n: int, mass=None, thrust_scale=None, thrust_poly=None, drag_coefficients=None,
           rates_transition_rate=None, thrust_transition_rate=None) -> np.ndarray:
    """[n, FPV_PHYS_INPUTS] float64 parameter sets: every argument None (the base value), a scalar, [n], or - thrust_poly [4] /
    [n, 4], drag_coefficients [3] / [n, 3] - one row per drone; `thrust_scale` multiplies the thrust cubic (motor strength)."""
    out = np.tile(base_inputs(cp), (n, 1))
    if mass is not None:
        out[:, _lib.PHYS_IN_MASS] = _cols(mass, n, 1, "mass")[:, 0]
    if thrust_poly is not None:
        out[:, _lib.PHYS_IN_C3:_lib.PHYS_IN_C3 + 4] = _cols(thrust_poly, n, 4, "thrust_poly")
    if thrust_scale is not None:
        out[:, _lib.PHYS_IN_C3:_lib.PHYS_IN_C3 + 4] *= _cols(thrust_scale, n, 1, "thrust_scale")
    if drag_coefficients is not None:
        out[:, _lib.PHYS_IN_CD_X:_lib.PHYS_IN_CD_X + 3] = _cols(drag_coefficients, n, 3, "drag_coefficients")
    if rates_transition_rate is not None:
        out[:, _lib.PHYS_IN_RATES_LAG] = _cols(rates_transition_rate, n, 1, "rates_transition_rate")[:, 0]
    if thrust_transition_rate is not None:
        out[:, _lib.PHYS_IN_THRUST_LAG] = _cols(thrust_transition_rate, n, 1, "thrust_transition_rate")[:, 0]
    return out


def derive(cp: _lib.FpvParams, sets: Optional[np.ndarray], n: Optional[int] = None) -> np.ndarray:
    """[FPV_PHYS_ROWS, n] float32 table columns of the parameter sets (None: n columns of the base parameters);
    a NaN cell takes the base value (fpv_physics_derive)."""
    if sets is not None:
        sets = np.ascontiguousarray(sets, dtype=np.float64)
        if sets.ndim != 2 or sets.shape[1] != INPUTS:
            raise ValueError(f"parameter sets are [n, {INPUTS}]")
        n = sets.shape[0]
    rows = np.empty((ROWS, int(n)), dtype=np.float32)
    _lib.check(_lib.lib().fpv_physics_derive(C.byref(cp), int(n), None if sets is None else sets.ctypes.data, rows.ctypes.data, int(n)))
    return rows


def sample(cp: _lib.FpvParams, seed: int, global_id0: int, n: int, mass: Sequence[float] = (1.0, 1.0),
           thrust: Sequence[float] = (1.0, 1.0), drag: Sequence[float] = (1.0, 1.0), rates_lag: Sequence[float] = (1.0, 1.0),
           thrust_lag: Sequence[float] = (1.0, 1.0)) -> np.ndarray:
    """[n, FPV_PHYS_INPUTS] float64 parameter sets of drones global_id0 .. global_id0 + n - 1: the base values times a factor
    drawn uniformly from (lo, hi) per drone - one for the mass, one for the whole thrust cubic, one per drag axis, one per
    low-pass rate (fpv_physics_sample: keyed by seed and global drone id only)."""
    ranges = np.ones((INPUTS, 2), dtype=np.float64)
    ranges[_lib.PHYS_IN_MASS] = mass
    ranges[_lib.PHYS_IN_C3:_lib.PHYS_IN_C3 + 4] = thrust
    ranges[_lib.PHYS_IN_CD_X:_lib.PHYS_IN_CD_X + 3] = drag
    ranges[_lib.PHYS_IN_RATES_LAG], ranges[_lib.PHYS_IN_THRUST_LAG] = rates_lag, thrust_lag
    out = np.empty((int(n), INPUTS), dtype=np.float64)
    _lib.check(_lib.lib().fpv_physics_sample(C.byref(cp), int(seed) & (2 ** 64 - 1), int(global_id0), int(n), ranges.ctypes.data,
                                             out.ctypes.data))
    return out
